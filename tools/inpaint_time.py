"""What masked inpainting costs per step on SDXL-base bf16 (synthetic weights), guided Euler, latent 128, batch 1, in one process on one
device:

  (a) the loop built without `inpaint`;
  (b) the loop built with `inpaint=True` and the mask all ones ("off": one early-exit launch per step);
  (c) the same loop with the left half kept (half the pixels are rewritten every step).

    python tools/inpaint_time.py [--spec sdxl|tiny] [--steps 20] [--runs 7] [--out profiles/inpaint_time.json]

The two captured loop graphs are replayed in turn, (a) (b) (c) (a) ..., after one warm-up round; each run is one replay (host clock
around a device synchronise), medians over --runs with min and max.  `off_delta_us_per_step` = (b) - (a) and `half_delta_us_per_step` =
(c) - (a) are the added time per step.  `blend_*_us` is the kernel alone on the loop's own buffers at mask all ones, half kept and all
kept: device events around one replay of a captured graph of 200 launches (kernel boundaries included, the host's launch path not),
median of 5 replays.  `copy_same_bytes_us` is a device-to-device copy of the bytes the all-kept launch moves (init and noise read, the
fp32 latent and both row blocks of the bf16 input written, the mask read), timed the same way; `traffic_floor_us` is those bytes at
6.3 TB/s."""
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
    """Device time per launch inside a replayed graph of n launches (device events around one replay; median of 5 replays): the
    kernel and its boundary in a graph, as the loop runs it, without the host's launch path."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize(dev)
        out.append(a.elapsed_time(b) / n * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    spec, side = (SDXL_BASE, 128) if args.spec == "sdxl" else (TINY, 16)
    gm = optimize_model(build(spec, dt, dev), cuda_graph=False)
    x = synth.denoise_inputs(2, side, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    kw = dict(cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim, guidance_scale=5.0, mode="loop")
    ones = torch.ones(side, side)
    half = ones.clone()
    half[:, :side // 2] = 0.0
    with torch.no_grad():
        plain = DenoiseLoop(gm, 1, side, dt, dev, euler_discrete_tables(args.steps), **kw)
        inp = DenoiseLoop(gm, 1, side, dt, dev, euler_discrete_tables(args.steps), inpaint=True, **kw)
        for loop in (plain, inp):
            loop.set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
        noise = synth.normal("inpaint.noise", (1, 4, side, side), 7, dev)
        init = synth.normal("inpaint.init", (1, 4, side, side), 8, dev) * 0.8
        names = ("plain", "inpaint_mask_ones", "inpaint_half_kept")
        times = {k: [] for k in names}
        finals = {}
        for i in range(args.runs + 1):                             # (round 0 captures and warms both graphs up)
            for name, loop, mask in ((names[0], plain, None), (names[1], inp, ones), (names[2], inp, half)):
                if mask is not None:
                    loop.set_inpaint(init, mask)
                loop.set_noise(noise)
                t = timed(lambda: loop.run_steps(args.steps), dev)
                finals[name] = loop.latent.clone()
                if i:
                    times[name].append(t / args.steps)
        finite = all(bool(torch.isfinite(v).all()) for v in finals.values())
        off_is_plain = bool(torch.equal(finals[names[0]], finals[names[1]]))
        kept_is_init = bool(torch.equal(finals[names[2]][:, :, :, :side // 2], init[:, :, :, :side // 2]))
        # the kernel alone, on the loop's own buffers
        launch = lambda: ops.inpaint_blend(inp.latent, inp.x_step, inp.inpaint_init, inp.inpaint_noise, inp.inpaint_mask, inp.sigma_next,
                                           inp.in_scale, inp.step_ids[0:1], inp.inpaint_thr)
        blend_us = {}
        for name, mask in (("ones", ones), ("half", half), ("zeros", torch.zeros(side, side))):
            inp.set_inpaint(init, mask)
            blend_us[name] = kernel_us(launch, dev)
        lat_bytes = inp.latent.numel() * 4
        moved = 3 * lat_bytes + inp.x_step.numel() * inp.x_step.element_size() + inp.inpaint_mask.numel() * 4
        src = torch.zeros(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy_us = kernel_us(lambda: dst.copy_(src), dev)
    med = {k: statistics.median(v) for k, v in times.items()}
    line = json.dumps({
        "tool": "inpaint_time", "spec": args.spec, "dtype": "bf16", "latent": side, "batch": 1, "guided": True, "steps": args.steps,
        "runs": args.runs,
        **{f"{k}_ms_per_step": round(med[k], 4) for k in names},
        **{f"{k}_min_max": [round(min(times[k]), 4), round(max(times[k]), 4)] for k in names},
        "off_delta_us_per_step": round((med[names[1]] - med[names[0]]) * 1e3, 2),
        "half_delta_us_per_step": round((med[names[2]] - med[names[0]]) * 1e3, 2),
        "blend_mask_ones_us": round(blend_us["ones"], 2), "blend_half_kept_us": round(blend_us["half"], 2),
        "blend_all_kept_us": round(blend_us["zeros"], 2), "copy_same_bytes_us": round(copy_us, 2), "bytes_all_kept": moved,
        "traffic_floor_us": round(moved / HBM_ACHIEVABLE * 1e6, 3),
        "off_is_plain_bit_for_bit": off_is_plain, "kept_half_is_init_bit_for_bit": kept_is_init, "finite": finite})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
