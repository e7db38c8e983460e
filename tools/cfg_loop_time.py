"""Guided denoise loop vs the same loop without guidance at batch 2, SDXL-base 1024 px (latent 128), bf16, mode loop, one process.

    python tools/cfg_loop_time.py [--runs 5] [--rescale] [--steps 50] [--out cfg_loop_time.json]

Both loops run the UNet at batch 2 over the same compiled module; they differ only in the update after it: `euler_kernel` over
the batch-2 latent (unguided) against `cfg_euler_kernel` (+ `cfg_stats_kernel` with --rescale) over the batch-1 latent.
Whole 50-step trajectories (one graph launch each) are timed alternately, A B A B ..., after one warm-up trajectory of each,
host clock around a device synchronise.  A second part times the update ops alone: 200 calls captured in one graph per op,
so the per-call figure carries no host launch cost.  Prints one JSON line.
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
from stabletriton_amd.unet import SDXL_BASE, UNet2DConditionModel  # noqa: E402


def graph_us(fn, calls=200, reps=5):
    """Per-call time of `fn` from `calls` captured launches replayed `reps` times (median of the replays)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--rescale", action="store_true", help="the guided loop also applies guidance rescale 0.7")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    with torch.device("meta"):
        m = UNet2DConditionModel(SDXL_BASE)
    m = m.to_empty(device=dev).to(dt).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    gm = optimize_model(m, cuda_graph=False)
    tables = euler_discrete_tables(args.steps)
    x = synth.denoise_inputs(2, args.latent, 1234, device=dev)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    loops = {"plain_b2": DenoiseLoop(gm, 2, args.latent, dt, dev, tables, mode="loop"),
             "cfg_b1": DenoiseLoop(gm, 1, args.latent, dt, dev, tables, mode="loop", guidance_scale=5.0,
                                   guidance_rescale=0.7 if args.rescale else None)}
    loops["plain_b2"].set_conditioning(*cond)
    loops["cfg_b1"].set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
    noise = {"plain_b2": x["latent"], "cfg_b1": x["latent"][:1]}
    times = {k: [] for k in loops}
    with torch.no_grad():
        for k, lp in loops.items():
            lp.capture()
            lp.denoise(noise[k])                                   # warm-up trajectory
        for _ in range(args.runs):
            for k, lp in loops.items():
                lp.set_noise(noise[k])
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                lp.run_steps(args.steps)
                torch.cuda.synchronize(dev)
                times[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
        finite = all(bool(torch.isfinite(lp.latent).all()) for lp in loops.values())

        # the update ops alone, at the loops' shapes
        p, c = loops["plain_b2"], loops["cfg_b1"]
        eps2 = torch.randn_like(p.x_in)
        lat2, lat1 = p.latent.clone(), c.latent.clone()
        nxt = torch.empty_like(p.x_in)
        ids = p.step_ids[10:11]
        op_us = {"euler_step_b2": graph_us(lambda: ops.euler_step(lat2, eps2, nxt, p.dsigma, p.in_scale, ids)),
                 "cfg_euler_step_b1": graph_us(lambda: ops.cfg_euler_step(lat1, eps2, nxt, c.dsigma, c.in_scale, c.guidance, ids))}
        ws = ops.cfg_workspace(lat1)
        resc = torch.full_like(c.dsigma, 0.7)
        op_us["cfg_euler_step_b1_rescale"] = graph_us(
            lambda: ops.cfg_euler_step(lat1, eps2, nxt, c.dsigma, c.in_scale, c.guidance, ids, rescale=resc, workspace=ws))

    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"what": f"SDXL-base {args.latent * 8} px bf16, mode loop, {args.steps} steps: guided bs=1"
                   + (" (rescale 0.7)" if args.rescale else "") + " vs unguided bs=2, same process, alternating",
           "ms_per_step_median": {k: round(v, 3) for k, v in med.items()},
           "ms_per_step_all": {k: [round(t, 3) for t in v] for k, v in times.items()},
           "guided_it_per_s": round(1e3 / med["cfg_b1"], 2),
           "guided_minus_plain_us_per_step": round((med["cfg_b1"] - med["plain_b2"]) * 1e3, 1),
           "update_op_us_in_graph": {k: round(v, 2) for k, v in op_us.items()},
           "finite": finite}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
