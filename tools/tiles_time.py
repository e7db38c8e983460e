"""What tiling costs per step on SDXL-base bf16 (synthetic weights), guided Euler, in one process:

  (a) the tiled loop: canvas 128 x 256 latent, window 128, stride 64 - T = 3 windows, six UNet rows;
  (b) an untiled loop at latent 128 with batch 3: the same six UNet rows, on code that does not know of tiles.

    python tools/tiles_time.py [--spec sdxl|tiny] [--steps 20] [--runs 7] [--out profiles/tiles_time.json]

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/tiles_time.py --trace [--spec sdxl|tiny]

The two captured loop graphs are replayed alternately (one warm-up replay of each first); each run is one replay (host clock around a
device synchronise), medians over --runs with min and max.  `delta_ms_per_step` = (a) - (b): the blend and gather launches with their
two launch boundaries, and the update kernel reading its prediction and writing its next input at canvas size beside the windows'.
`tile_blend_us` / `tile_gather_us` are device events around 200 back-to-back launches of each kernel on the loop's own buffers (launch
gaps included), with the traffic floor of one of them - windows and canvas moved once at 6.3 TB/s - beside them.  Trace mode builds the
same buffers without the UNet, launches each kernel 200 times and prints one line: run it under rocprofv3 and read the two kernels'
own times from the statistics."""
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


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def kernel_us(fn, dev, n=200):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="launch the two kernels alone (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    spec, win = (SDXL_BASE, 128) if args.spec == "sdxl" else (TINY, 16)
    canvas = (win, 2 * win)
    if args.trace:
        loop = DenoiseLoop(lambda *a, **k: None, 1, canvas, dt, dev, euler_discrete_tables(args.steps), cross_dim=spec.cross_dim,
                           pooled_dim=spec.pooled_dim, guidance_scale=5.0, mode="eager", tile_hw=win, tile_stride=win // 2)
        g = loop.tile_grid
        eps = torch.randn_like(loop.x_in)
        for _ in range(200):
            ops.tile_blend(eps, loop.eps_canvas, loop.tile_weights, g.ys, g.xs, g.wrap_w)
            ops.tile_gather(loop.x_step, loop.x_in, g.ys, g.xs, g.wrap_w)
        torch.cuda.synchronize(dev)
        print(json.dumps({"tool": "tiles_time", "trace": True, "launches_each": 200, "finite": bool(torch.isfinite(loop.eps_canvas).all())}))
        return
    gm = optimize_model(build(spec, dt, dev), cuda_graph=False)
    x = synth.denoise_inputs(2, win, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    kw = dict(cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim, guidance_scale=5.0, mode="loop")
    with torch.no_grad():
        tiled = DenoiseLoop(gm, 1, canvas, dt, dev, euler_discrete_tables(args.steps), tile_hw=win, tile_stride=win // 2, **kw)
        tiled.set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
        plain = DenoiseLoop(gm, 3, win, dt, dev, euler_discrete_tables(args.steps), **kw)
        plain.set_conditioning(*(c[1:2].expand(3, *c.shape[1:]) for c in cond), *(c[0:1].expand(3, *c.shape[1:]) for c in cond))
        T = tiled.tile_grid.T
        assert tiled.x_in.shape == plain.x_in.shape and T == 3
        n_canvas = synth.normal("tiles.canvas", (1, 4) + canvas, 7, dev)
        n_plain = synth.normal("tiles.plain", (3, 4, win, win), 7, dev)
        times = {"tiled": [], "untiled": []}
        finite = True
        for i in range(args.runs + 1):                             # (round 0 captures and warms both graphs up)
            for name, loop, noise in (("tiled", tiled, n_canvas), ("untiled", plain, n_plain)):
                loop.set_noise(noise)
                t = timed(lambda: loop.run_steps(args.steps), dev)
                finite = finite and bool(torch.isfinite(loop.latent).all())
                if i:
                    times[name].append(t / args.steps)
        g = tiled.tile_grid
        eps = torch.randn_like(tiled.x_in)
        blend_us = kernel_us(lambda: ops.tile_blend(eps, tiled.eps_canvas, tiled.tile_weights, g.ys, g.xs, g.wrap_w), dev)
        gather_us = kernel_us(lambda: ops.tile_gather(tiled.x_step, tiled.x_in, g.ys, g.xs, g.wrap_w), dev)
    med = {k: statistics.median(v) for k, v in times.items()}
    win_bytes, canvas_bytes = tiled.x_in.numel() * 2, tiled.x_step.numel() * 2
    line = json.dumps({
        "tool": "tiles_time", "spec": args.spec, "dtype": "bf16", "canvas": list(canvas), "window": win, "stride": win // 2, "windows": T,
        "unet_rows": int(tiled.x_in.shape[0]), "steps": args.steps, "runs": args.runs,
        "tiled_ms_per_step": round(med["tiled"], 4), "tiled_min_max": [round(min(times["tiled"]), 4), round(max(times["tiled"]), 4)],
        "untiled_ms_per_step": round(med["untiled"], 4), "untiled_min_max": [round(min(times["untiled"]), 4), round(max(times["untiled"]), 4)],
        "delta_ms_per_step": round(med["tiled"] - med["untiled"], 4),
        "delta_percent_of_step": round(100.0 * (med["tiled"] - med["untiled"]) / med["untiled"], 3),
        "tile_blend_us": round(blend_us, 2), "tile_gather_us": round(gather_us, 2),
        "traffic_floor_us": round((win_bytes + canvas_bytes) / HBM_ACHIEVABLE * 1e6, 3),
        "finite": finite})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
