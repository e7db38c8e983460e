"""What StyleAligned costs on SDXL-base bf16 (synthetic weights), on one device.

1. Per self-attention site shape with the loop's rows, B = 4 = [negative(2) | positive(2)], per = 2 (T = 4096 with 10 heads, 1024 with
   20; q / k / v column slices of one fused buffer): the AdaIN launch pair (ops.style_adain on q and k) and ops.attention_shared, each
   with the gate on and gated off, beside ops.attention on the same rows.  Each variant is a captured graph of --launches calls, the
   graphs replayed in turn, device events around a replay, after one warm-up round; medians over --runs with min and max, in
   microseconds per call.  The pair's bytes: the statistics launch reads 2 slices x B rows, the affine reads and writes 2 slices x the
   B / 2 other rows, T * C 16-bit values each.  `--sites-only --site T,H` runs this part alone for one shape: under a kernel trace
   (`rocprofv3 --kernel-trace --stats -- python tools/style_aligned_time.py --sites-only --pair-only --site 4096,10`) the two AdaIN kernels are timed
   one by one; `stats_bytes` / `apply_bytes` in the output are what each moves.
2. ms/step of the guided Euler loop at 1024 x 1024 (latent 128), batch 2, --steps steps: the loop without the flag on a UNet compiled
   without the sites, and StyleAligned loops on, off (`set_style_aligned(None)`: the plain launches are captured) and on at the last
   step alone (19 of 20 steps gated off on the device); the captured loop graphs are replayed in turn, host clock around a device
   synchronise.  `--parent-root DIR` (a built checkout of the commit before the feature) also runs the loop
   without the flag from that tree, in a child process before and after this process's own measurements (`--plain-only --root DIR`).

    python tools/style_aligned_time.py [--spec sdxl|tiny] [--steps 20] [--runs 7] [--parent-root DIR] [--out profiles/style_aligned_time.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

PEAK_HBM_GBS = 8000.0          # HBM3E spec (bench.py)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--sites-only", action="store_true")
    ap.add_argument("--site", default=None, help="T,H: this site shape alone")
    ap.add_argument("--pair-only", action="store_true", help="with --sites-only: time the gated-on AdaIN pair alone")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


ARGS = parse()
sys.path.insert(0, os.path.abspath(ARGS.root))      # the tree whose package is measured

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
    B, per, C = 4, 2, H * 64
    scale = 64 ** -0.5
    fused = (synth.normal(f"style_aligned_time.qkv{T}", (B, T, 3 * C), 3, dev)).to(dt)
    q, k, v = fused[..., :C], fused[..., C:2 * C], fused[..., 2 * C:]
    ws = ops.style_adain_workspace(B, T, C, 2, dev)
    off = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev))
    variants = {
        "adain_pair": lambda: ops.style_adain((q, k), per, workspace=ws),
        "adain_pair_off": lambda: ops.style_adain((q, k), per, gate=off, workspace=ws),
        "attention_shared": lambda: ops.attention_shared(q, k, v, H, scale, per),
        "attention_shared_off": lambda: ops.attention_shared(q, k, v, H, scale, per, gate=off),
        "attention": lambda: ops.attention(q, k, v, H, scale),
    }
    if ARGS.pair_only:                                             # (under a kernel trace: every AdaIN launch in the trace is a gated-on one)
        variants = {"adain_pair": variants["adain_pair"]}
    graphs = {name: graph_of(fn, dev, launches) for name, fn in variants.items()}
    times = {name: [] for name in variants}
    for i in range(runs + 1):                                      # (round 0 warms up)
        for name, g in graphs.items():
            t = replay_us(g, dev, launches)
            if i:
                times[name].append(t)
    out = {"T": T, "H": H, "B": B, "per": per, "finite": bool(torch.isfinite(fused).all())}
    for name, ts in times.items():
        out[f"{name}_us"] = round(statistics.median(ts), 2)
        out[f"{name}_min_max"] = [round(min(ts), 2), round(max(ts), 2)]
    out["stats_bytes"] = 2 * T * C * 2 * B
    out["apply_bytes"] = 2 * T * C * 2 * 2 * (B - B // per)
    out["adain_pair_GBs"] = round((out["stats_bytes"] + out["apply_bytes"]) / (out["adain_pair_us"] * 1e-6) / 1e9, 1)
    out["adain_pair_share_of_hbm_peak"] = round(out["adain_pair_GBs"] / PEAK_HBM_GBS, 4)
    return out


def loops(args, dev, dt, spec, side, style_sites):
    """ms/step lists and final latents of the plain loop and, with `style_sites`, of the StyleAligned loop on and off."""
    x = synth.denoise_inputs(2, side, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    kw = dict(cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim, guidance_scale=5.0, mode="loop")
    plain = DenoiseLoop(optimize_model(build(spec, dt, dev), cuda_graph=False), 2, side, dt, dev, euler_discrete_tables(args.steps), **kw)
    rounds = [("plain", plain, None)]
    if style_sites:
        gm = optimize_model(build(spec, dt, dev), cuda_graph=False, style_aligned_layers=(".*",))
        # one loop per setting: going from on to off drops a loop's graph (set_style_aligned), and captures are not what is timed here.
        # "window_off": on at the last step only, so 19 of 20 steps run their sites gated off on the device
        for name, window in (("style_aligned_on", (0.0, 1.0)), ("style_aligned_off", (None,)), ("style_aligned_window_off", (0.96, 1.0))):
            loop = DenoiseLoop(gm, 2, side, dt, dev, euler_discrete_tables(args.steps), style_aligned=True, **kw)
            loop.set_style_aligned(*window)
            rounds.append((name, loop, None))
    for loop in {id(r[1]): r[1] for r in rounds}.values():
        loop.set_conditioning(*cond, *(c.flip(0) for c in cond))
    noise = synth.normal("style_aligned_time.noise", (2, 4, side, side), 7, dev)
    times = {r[0]: [] for r in rounds}
    finals = {r[0]: [] for r in rounds}
    for i in range(args.runs + 1):                                 # (round 0 captures and warms the graphs up)
        for name, loop, _ in rounds:
            loop.set_noise(noise)
            t = timed(lambda: loop.run_steps(args.steps), dev)
            finals[name].append(loop.latent.clone())
            if i:
                times[name].append(t / args.steps)
    return times, finals


def summary(ts):
    return {"ms_per_step": round(statistics.median(ts), 4), "min_max": [round(min(ts), 4), round(max(ts), 4)]}


def parent_plain(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--root", args.parent_root, "--spec", args.spec,
                        "--steps", str(args.steps), "--runs", str(args.runs)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"the parent tree's loop failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    args = ARGS
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    spec, side = (SDXL_BASE, 128) if args.spec == "sdxl" else (TINY, 32)
    with torch.no_grad():
        if args.plain_only:
            times, _ = loops(args, dev, dt, spec, side, False)
            print(json.dumps(summary(times["plain"])))
            return
        shapes = ((4096, 10), (1024, 20)) if args.spec == "sdxl" else ((256, 2),)
        if args.site:
            shapes = (tuple(int(v) for v in args.site.split(",")),)
        sites = [site(T, H, dev, dt, args.runs, args.launches) for T, H in shapes]
        if args.sites_only:
            print(json.dumps({"tool": "style_aligned_time", "sites": sites}))
            return
        parent = [parent_plain(args)] if args.parent_root else []
        times, finals = loops(args, dev, dt, spec, side, True)
        if args.parent_root:
            parent.append(parent_plain(args))
    names = tuple(times)
    med = {k: statistics.median(v) for k, v in times.items()}
    line = json.dumps({
        "tool": "style_aligned_time", "spec": args.spec, "dtype": "bf16", "latent": side, "batch": 2, "guided": True, "steps": args.steps,
        "runs": args.runs, "launches_per_graph": args.launches, "peak_hbm_GBs": PEAK_HBM_GBS, "sites": sites,
        **{k: summary(v) for k, v in times.items()},
        "parent_commit_plain_before_and_after": parent or "not measured",
        "on_over_off": round(med[names[1]] / med[names[2]], 4), "off_over_plain": round(med[names[2]] / med[names[0]], 4),
        "window_off_over_plain": round(med[names[3]] / med[names[0]], 4),
        "off_equals_plain_bits": bool(torch.equal(finals[names[2]][0], finals[names[0]][0])),
        "style_image_equals_plain_bits": bool(torch.equal(finals[names[1]][0][0], finals[names[0]][0][0])),
        "on_changes_the_other_image": not bool(torch.equal(finals[names[1]][0][1], finals[names[0]][0][1])),
        "every_loop_repeats_its_bits": all(bool(torch.equal(v, vs[0])) for vs in finals.values() for v in vs),
        "finite": all(bool(torch.isfinite(v).all()) for vs in finals.values() for v in vs)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
