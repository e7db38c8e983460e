"""What self-attention guidance costs on SDXL-base bf16 (synthetic weights), on one device.

1. At the real site shape (the middle block's first self-attention at latent 128: 1024 tokens, 20 heads, one recording entry): the
   column-sum launches (ops.attention_colsum: rows, columns, heads) beside ops.attention on the same rows, and the degrade launch
   (ops.sag_degrade) at latent 128.  Each is a captured graph of --launches calls, the graphs replayed in turn, device events around a
   replay, after one warm-up round; medians over --runs with min and max, in microseconds per call.
2. ms/step of the guided Euler loop at 1024 x 1024 (latent 128), batch 1, --steps steps, captured loop graphs replayed in turn, host
   clock around a device synchronise: a UNet compiled without `sag_layer`, one with the site in a loop without `sag_scale`, and
   `sag_scale=0.5`.  `--parent-root DIR` (a built checkout of the commit before the feature) also runs the first of them from that tree,
   in a child process before and after this process's own measurements (`--plain-only --root DIR`).

    python tools/sag_time.py [--spec sdxl|tiny] [--steps 20] [--runs 7] [--parent-root DIR] [--out profiles/sag_time.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--plain-only", action="store_true")
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


def kernels(T, H, side, dev, dt, runs, launches):
    C, scale = H * 64, 64 ** -0.5
    fused = synth.normal(f"sag_time.qkv{T}", (1, T, 3 * C), 3, dev).to(dt)
    q, k, v = fused[..., :C], fused[..., C:2 * C], fused[..., 2 * C:]
    A, ws = torch.zeros((1, T), device=dev), ops.attention_colsum_workspace(1, T, H, dev)
    cl = torch.channels_last
    lat = synth.normal("sag_time.latent", (1, 4, side, side), 5, dev).contiguous(memory_format=cl)
    eps = synth.normal("sag_time.eps", (1, 4, side, side), 6, dev).to(dt).contiguous(memory_format=cl)
    out, mask = torch.empty_like(eps), torch.zeros((1, side, side), device=dev)
    grid = (int(T ** 0.5), int(T ** 0.5))
    sig, step, par = torch.tensor([7.0], device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([1.0, 2.0], device=dev)
    variants = {"attention_colsum": lambda: ops.attention_colsum(q, k, H, scale, out=A, workspace=ws),
                "attention": lambda: ops.attention(q, k, v, H, scale),
                "sag_degrade": lambda: ops.sag_degrade(lat, eps, A, grid, sig, sig, step, par, out, mask)}
    graphs = {name: graph_of(fn, dev, launches) for name, fn in variants.items()}
    times = {name: [] for name in variants}
    for i in range(runs + 1):                                      # (round 0 warms up)
        for name, g in graphs.items():
            t = replay_us(g, dev, launches)
            if i:
                times[name].append(t)
    res = {"T": T, "H": H, "rows": 1, "latent": side, "colsum_total_over_T": round(float(A.sum()) / T, 6),
           "masked_share": round(float(mask.mean()), 4)}
    for name, ts in times.items():
        res[f"{name}_us"] = round(statistics.median(ts), 2)
        res[f"{name}_min_max"] = [round(min(ts), 2), round(max(ts), 2)]
    return res


def loops(args, dev, dt, spec, side, with_sag):
    x = synth.denoise_inputs(1, side, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    kw = dict(cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim, guidance_scale=5.0, mode="loop")
    tables = lambda: euler_discrete_tables(args.steps)
    rounds = [("plain", DenoiseLoop(optimize_model(build(spec, dt, dev), cuda_graph=False), 1, side, dt, dev, tables(), **kw))]
    if with_sag:
        gm = optimize_model(build(spec, dt, dev), cuda_graph=False, sag_layer=True)
        rounds.append(("site_compiled_in", DenoiseLoop(gm, 1, side, dt, dev, tables(), **kw)))
        rounds.append(("sag_on", DenoiseLoop(gm, 1, side, dt, dev, tables(), sag_scale=0.5, **kw)))
    for _, loop in rounds:
        loop.set_conditioning(*cond, *(c * 0.5 for c in cond))
    noise = synth.normal("sag_time.noise", (1, 4, side, side), 7, dev)
    times, finals = {r[0]: [] for r in rounds}, {r[0]: [] for r in rounds}
    for i in range(args.runs + 1):                                 # (round 0 captures and warms the graphs up)
        for name, loop in rounds:
            loop.set_noise(noise)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            loop.run_steps(args.steps)
            torch.cuda.synchronize(dev)
            finals[name].append(loop.latent.clone())
            if i:
                times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
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
    spec, side, shape = (SDXL_BASE, 128, (1024, 20)) if args.spec == "sdxl" else (TINY, 32, (64, 2))
    with torch.no_grad():
        if args.plain_only:
            print(json.dumps(summary(loops(args, dev, dt, spec, side, False)[0]["plain"])))
            return
        site = kernels(*shape, side, dev, dt, args.runs, args.launches)
        parent = [parent_plain(args)] if args.parent_root else []
        times, finals = loops(args, dev, dt, spec, side, True)
        if args.parent_root:
            parent.append(parent_plain(args))
    med = {k: statistics.median(v) for k, v in times.items()}
    line = json.dumps({
        "tool": "sag_time", "spec": args.spec, "dtype": "bf16", "latent": side, "batch": 1, "guided": True, "steps": args.steps,
        "runs": args.runs, "launches_per_graph": args.launches, "site": site, **{k: summary(v) for k, v in times.items()},
        "parent_commit_plain_before_and_after": parent or "not measured",
        "site_compiled_in_over_plain": round(med["site_compiled_in"] / med["plain"], 4), "sag_on_over_plain": round(med["sag_on"] / med["plain"], 4),
        "site_compiled_in_equals_plain_bits": bool(torch.equal(finals["site_compiled_in"][0], finals["plain"][0])),
        "sag_changes_the_result": not bool(torch.equal(finals["sag_on"][0], finals["plain"][0])),
        "every_loop_repeats_its_bits": all(bool(torch.equal(v, vs[0])) for vs in finals.values() for v in vs),
        "finite": all(bool(torch.isfinite(v).all()) for vs in finals.values() for v in vs)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
