"""What FreeU costs per step on SDXL-base bf16 at latent 128: the captured 50-step loop of a module compiled with
`freeu=True` against one compiled without, same weights, alternated in one process.

    python tools/freeu_time.py [--spec sdxl|tiny] [--steps 50] [--runs 5] [--out freeu_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/freeu_time.py --trace on|off [--guided] [--trace-steps 4]

Timing mode, per batch form (bs = 1 unguided; guided = 2 UNet rows), one JSON object:
  off_ms_per_step       the module without FreeU sites (the product's default graph)
  neutral_ms_per_step   freeu=True, neutral parameters: the sites run (two launches each, copies) and change nothing
  v1_ms_per_step / v2_ms_per_step   freeu=True at the SDXL values, version 1 / 2;  *_delta_ms: minus off_ms_per_step
  floor_us              the sites' own traffic - both tensors read twice and written once, from the shapes - at 6.3 TB/s
Each run is one replay of the loop graph (host clock around a device synchronise) after one warm-up replay of each;
medians over --runs, with min and max of the off / v1 runs to show the spread.

Trace mode runs ONE module only (`on`: freeu=True at the SDXL values, version 1; `off`), eagerly, for --trace-steps steps
and prints nothing but a line with the step count: run it under rocprofv3 and read the two FreeU kernels' time and the
total number of dispatches from the statistics; (dispatches_on - dispatches_off) / steps is the launches a step gains.
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

from stabletriton_amd import synth  # noqa: E402
from stabletriton_amd.optimization import optimize_model  # noqa: E402
from stabletriton_amd.pipeline import DenoiseLoop  # noqa: E402
from stabletriton_amd.scheduler import euler_discrete_tables  # noqa: E402
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s
SDXL_VALUES = dict(s1=0.9, s2=0.2, b1=1.3, b2=1.4)


def site_shapes(spec, latent):
    """(C_h, C_skip, pixels) of the sites of decoder stages 0 and 1."""
    w, n = spec.widths, len(spec.widths)
    skips = [w[0]]
    for lvl in range(n):
        skips += [w[lvl]] * spec.resnets_per_level + ([w[lvl]] if lvl < n - 1 else [])
    out, c_prev = [], w[-1]
    for i, lvl in enumerate(reversed(range(n))):
        side = latent >> lvl
        for _ in range(spec.resnets_per_level + 1):
            if i < 2:
                out.append((c_prev, skips[-1], side * side))
            skips.pop()
            c_prev = w[lvl]
    return out


def floor_us(spec, latent, rows, itemsize=2):
    elems = sum((ch + cs) * px for ch, cs, px in site_shapes(spec, latent)) * rows
    return 3 * elems * itemsize / HBM_ACHIEVABLE * 1e6


def build(spec, dt, dev):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec)
    m = m.to_empty(device=dev).to(dt).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


def make_loop(gm, spec, latent, dt, dev, steps, guided, mode, x):
    loop = DenoiseLoop(gm, 1, latent, dt, dev, euler_discrete_tables(steps), cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim,
                       guidance_scale=5.0 if guided else None, mode=mode)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    if guided:
        loop.set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
    else:
        loop.set_conditioning(*(c[1:2] for c in cond))
    return loop


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace", choices=("on", "off"), default=None)
    ap.add_argument("--trace-steps", type=int, default=4)
    ap.add_argument("--guided", action="store_true", help="trace mode: the guided (2-row) form")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    spec, latent = (SDXL_BASE, 128) if args.spec == "sdxl" else (TINY, 16)
    m = build(spec, dt, dev)
    x = synth.denoise_inputs(2, latent, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    noise = x["latent"][:1]
    if args.trace is not None:
        gm = optimize_model(m, cuda_graph=False, freeu=args.trace == "on")
        with torch.no_grad():
            loop = make_loop(gm, spec, latent, dt, dev, args.trace_steps, args.guided, "eager", x)
            if args.trace == "on":
                loop.set_freeu(**SDXL_VALUES)
            out = loop.denoise(noise)
        torch.cuda.synchronize(dev)
        print(json.dumps({"tool": "freeu_time", "trace": args.trace, "guided": args.guided, "steps": args.trace_steps,
                          "finite": bool(torch.isfinite(out).all())}))
        return
    off = optimize_model(m, cuda_graph=False)
    on = optimize_model(m, cuda_graph=False, freeu=True)
    results = []
    with torch.no_grad():
        for guided in (False, True):
            l_off = make_loop(off, spec, latent, dt, dev, args.steps, guided, "loop", x)
            l_on = make_loop(on, spec, latent, dt, dev, args.steps, guided, "loop", x)
            settings = {"off": None, "neutral": None, "v1": dict(SDXL_VALUES, version=1), "v2": dict(SDXL_VALUES, version=2)}
            times = {k: [] for k in settings}
            finite = True
            for i in range(args.runs + 1):                         # (round 0 captures and warms both graphs up)
                for name, fu in settings.items():
                    loop = l_off if name == "off" else l_on
                    if name != "off":
                        loop.set_freeu(None) if fu is None else loop.set_freeu(**fu)
                    loop.set_noise(noise)
                    t = timed(lambda: loop.run_steps(args.steps), dev)
                    finite = finite and bool(torch.isfinite(loop.latent).all())
                    if i:
                        times[name].append(t / args.steps)
            med = {k: statistics.median(v) for k, v in times.items()}
            results.append({"guided": guided, "unet_rows": 2 if guided else 1,
                            "off_ms_per_step": round(med["off"], 4), "off_min_max": [round(min(times["off"]), 4), round(max(times["off"]), 4)],
                            "neutral_ms_per_step": round(med["neutral"], 4), "neutral_delta_ms": round(med["neutral"] - med["off"], 4),
                            "v1_ms_per_step": round(med["v1"], 4), "v1_min_max": [round(min(times["v1"]), 4), round(max(times["v1"]), 4)],
                            "v1_delta_ms": round(med["v1"] - med["off"], 4),
                            "v2_ms_per_step": round(med["v2"], 4), "v2_delta_ms": round(med["v2"] - med["off"], 4),
                            "floor_us": round(floor_us(spec, latent, 2 if guided else 1), 1), "finite": finite})
    line = json.dumps({"tool": "freeu_time", "spec": args.spec, "dtype": "bf16", "latent": latent, "steps": args.steps, "runs": args.runs,
                       "sites": [list(s) for s in site_shapes(spec, latent)], "results": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
