"""What ControlNet costs per step on SDXL-base bf16 at 1024 x 1024 (latent 128), bs = 1, guided (2 UNet rows), mode loop: three
variants of the captured loop, same weights, alternated in one process.

    python tools/controlnet_time.py [--spec sdxl|tiny] [--steps 20] [--runs 5] [--out profiles/controlnet_time.json]

One JSON object:
  a_ms_per_step   (a) a UNet compiled WITHOUT sites: the default graph
  b_ms_per_step   (b) sites compiled in, no branch, scale 0: one launch per step that reads its scale and leaves;   b_minus_a_ms
  c_ms_per_step   (c) the compiled branch + the sites at scale 0.8 in ONE grouped launch;                           c_minus_a_ms
  *_min_max       min and max over the runs: the spread the deltas are to be read against
  floor_us        the sites' own traffic - x read and written, the residuals read: 3 x tensor bytes - at 6.3 TB/s
  kernel          the launch alone on the sites' shapes (statistics rewritten where 256 rows per tile divide the image): microseconds
                  per launch, grouped and as one launch per site, from device events around one replay of a graph of --kernel-iters
                  launches (buffers resident in the caches; the boundary between two launches is inside the figure), and the ratio
                  of the grouped launch to the floor
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
from stabletriton_amd.controlnet import ControlNetXL  # noqa: E402
from stabletriton_amd.optimization import optimize_model  # noqa: E402
from stabletriton_amd.pipeline import DenoiseLoop  # noqa: E402
from stabletriton_amd.scheduler import euler_discrete_tables  # noqa: E402
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s


def build(cls, spec, dt, dev, seed):
    with torch.device("meta"):
        m = cls(spec)
    m = m.to_empty(device=dev).to(dt).eval().requires_grad_(False)
    synth.fill_module_(m, seed)
    return m


def make_loop(gm, spec, latent, dt, dev, steps, x, branch=None):
    loop = DenoiseLoop(gm, 1, latent, dt, dev, euler_discrete_tables(steps), cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim,
                       guidance_scale=5.0, mode="loop", controlnet=branch)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    loop.set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
    return loop


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def graph_us(fn, dev, iters):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()                                 # (captured: the host's launch rate is not what is measured)
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    g.replay()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) * 1e3 / iters


def kernel_alone(shapes, rows, dt, dev, iters):
    """All sites at scale 0.8: one grouped launch against one launch per site."""
    table = torch.full((1,), 0.8, dtype=torch.float32, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    xs, rs, sts = [], [], []
    for c, h, w in shapes:
        xs.append(torch.zeros((rows, c, h, w), dtype=dt, device=dev).contiguous(memory_format=torch.channels_last))
        rs.append(torch.full((rows, c, h, w), 2.0 ** -10, dtype=dt, device=dev).contiguous(memory_format=torch.channels_last))
        srows = 256 if (h * w) % 256 == 0 else 0
        sts.append(ops.ColStats(torch.zeros((rows * h * w // srows, c, 2), dtype=torch.float32, device=dev), srows, c) if srows else None)
    grouped = graph_us(lambda: ops.residual_add_grouped(xs, rs, table, step, sts), dev, iters)
    single = graph_us(lambda: [ops.residual_add(x, r, table, step, st) for x, r, st in zip(xs, rs, sts)], dev, iters)
    floor = 3 * rows * sum(c * h * w for c, h, w in shapes) * xs[0].element_size() / HBM_ACHIEVABLE * 1e6
    return {"sites": len(shapes), "grouped_us": round(grouped, 2), "one_launch_per_site_us": round(single, 2), "floor_us": round(floor, 2),
            "grouped_over_floor": round(grouped / floor, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    spec, latent = (SDXL_BASE, 128) if args.spec == "sdxl" else (TINY, 16)
    m = build(UNet2DConditionModel, spec, dt, dev, 0)
    net = build(ControlNetXL, spec, dt, dev, 3)
    x = synth.denoise_inputs(2, latent, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    noise = x["latent"][:1]
    without = optimize_model(m, cuda_graph=False)
    sites = optimize_model(m, cuda_graph=False, controlnet=True)
    branch = optimize_model(net, cuda_graph=False)
    state = sites.controlnet
    shapes = state.site_shapes(latent)
    cond = synth.normal("controlnet.time.cond", (1, spec.widths[0], latent, latent), 5).to(dev, dt)
    times = {k: [] for k in "abc"}
    finite = True
    with torch.no_grad():
        loops = {"a": make_loop(without, spec, latent, dt, dev, args.steps, x), "b": make_loop(sites, spec, latent, dt, dev, args.steps, x),
                 "c": make_loop(sites, spec, latent, dt, dev, args.steps, x, branch)}
        loops["c"].set_controlnet(cond, 0.8)
        for name in "abc":
            loops[name].capture()
        for i in range(args.runs + 1):                             # (round 0 warms the graphs up)
            for name in "abc":
                loop = loops[name]
                loop.set_noise(noise)
                t = timed(lambda: loop.run_steps(args.steps), dev)
                finite = finite and bool(torch.isfinite(loop.latent).all())
                if i:
                    times[name].append(t / args.steps)
        kernel = kernel_alone(shapes, 2, dt, dev, args.kernel_iters)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"tool": "controlnet_time", "spec": args.spec, "dtype": "bf16", "latent": latent, "unet_rows": 2, "steps": args.steps,
           "runs": args.runs, "sites": [list(s) for s in shapes], "finite": finite,
           "floor_us": kernel["floor_us"], "kernel": kernel}
    for k in "abc":
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
