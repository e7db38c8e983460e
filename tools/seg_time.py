"""What smoothed energy guidance costs per step on SDXL-base bf16 at latent 128 (1024 x 1024 px), Euler 50, guided, sites ("mid",):
captured loops over modules with the same weights, alternated in one process; then the blur and the blurred-tail attention alone.

    python tools/seg_time.py [--spec sdxl|tiny] [--steps 50] [--runs 5] [--out seg_time.json]

One JSON object.  "loops", milliseconds per step (one replay of the loop graph, host clock around a device synchronise, after one
warm-up replay of each; medians over --runs, with min and max):
  seg_inf_3b     CFG + SEG at sigma = infinity: rows [negative | positive | perturbed], the ten mid-block self-attentions of the
                 perturbed row run with their queries' spatial mean
  seg_10_3b      the same graph after set_seg(sigma=10) (the row is data: the same launches, 33 taps per pass on the 32 x 32 grid)
  plain_3b       the 3B loop with chunks = 0: the same rows, no perturbation (one attention launch per site)
  pag_3b         CFG + PAG on a module compiled with pag_layers=("mid",): the perturbed row's ten attentions are copies
seg_*_3b against plain_3b is what SEG adds per step: at each of the ten sites the blur launch and a second attention launch (the
batch of three splits into two and one).  "per_site_us" is that difference over the number of sites.
"blur": st_seg_blur alone on the tail's queries (1, 1024, 1280) bf16, the first column block of a fused q|k|v buffer, at both
sigmas: microseconds per call (device events around --reps back-to-back calls) against its traffic floor, the bytes read plus the
bytes written (2.6 MB each way) at 6.3 TB/s.  The buffers stay in the caches between calls: a lower bound of what the kernel takes
behind a q|k|v GEMM, not an HBM measurement.  "attention": ops.attention on all three entries in one launch against ops.attention_seg
with one tail entry (two attention launches and the blur).
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

from stabletriton_amd import ops, seg, synth  # noqa: E402
from stabletriton_amd.optimization import optimize_model  # noqa: E402
from stabletriton_amd.pipeline import DenoiseLoop  # noqa: E402
from stabletriton_amd.scheduler import euler_discrete_tables  # noqa: E402
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s
G, S = 5.0, 3.0
INF = float("inf")


def build(spec, dt, dev):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec)
    m = m.to_empty(device=dev).to(dt).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


def make_loop(gm, spec, latent, dt, dev, steps, x, **kw):
    loop = DenoiseLoop(gm, 1, latent, dt, dev, euler_discrete_tables(steps), cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim,
                       guidance_scale=G, mode="loop", **kw)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    loop.set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
    return loop


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def event_us(fn, reps, dev):
    """Microseconds per call of `fn`, device events around `reps` back-to-back calls (after `reps` warm-up calls)."""
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e3 / reps


def kernels_alone(dev, reps, grid, heads):
    h, w = grid
    B, T, D = 3, h * w, 64
    C = heads * D
    qkv = torch.randn((B, T, 3 * C), device=dev, dtype=torch.bfloat16)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    nbytes = 2 * T * C * 2
    blur, att = {}, {"shape": [B, T, heads, D], "attention_us_per_call": round(event_us(lambda: ops.attention(q, k, v, heads, D ** -0.5), reps, dev), 2)}
    for name, sigma in (("inf", INF), ("10", 10.0)):
        row = torch.tensor(seg.param_row(sigma, h, w), dtype=torch.float32, device=dev)
        us = event_us(lambda: ops.seg_blur(q[2:], grid, row), reps, dev)
        blur["sigma_" + name] = {"us_per_call": round(us, 2), "taps": int(row[1]) if sigma != INF else 0}
        att[f"attention_seg_tail1_sigma_{name}_us_per_call"] = round(event_us(lambda: ops.attention_seg(q, k, v, heads, D ** -0.5, 1, grid, row), reps, dev), 2)
    blur.update(shape=[1, T, C], dtype="bf16", bytes=nbytes, floor_us=round(nbytes / HBM_ACHIEVABLE * 1e6, 2))
    return blur, att


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    spec, latent = (SDXL_BASE, 128) if args.spec == "sdxl" else (TINY, 16)
    x = synth.denoise_inputs(2, latent, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    noise = x["latent"][:1]
    gm = optimize_model(build(spec, dt, dev), cuda_graph=False, seg_layers=("mid",))
    gm_pag = optimize_model(build(spec, dt, dev), cuda_graph=False, pag_layers=("mid",))
    sites = gm.rewrite_stats["seg_sites"]
    with torch.no_grad():
        seg_loop = make_loop(gm, spec, latent, dt, dev, args.steps, x, seg_scale=S, seg_sigma=INF)
        plain = make_loop(gm, spec, latent, dt, dev, args.steps, x, seg_scale=S)
        plain._perturbed_chunks = 0              # the same 3B rows and update, every attention ordinary (set before its capture)
        pag_loop = make_loop(gm_pag, spec, latent, dt, dev, args.steps, x, pag_scale=S)
        # (name, loop, sigma to set before the run: the two SEG entries are ONE captured graph under two parameter rows)
        order = [("seg_inf_3b", seg_loop, INF), ("seg_10_3b", seg_loop, 10.0), ("plain_3b", plain, None), ("pag_3b", pag_loop, None)]
        times = {name: [] for name, _, _ in order}
        finite = True
        graphs = set()
        for i in range(args.runs + 1):                             # (round 0 captures and warms every graph up)
            for name, loop, sigma in order:
                if sigma is not None:
                    loop.set_seg(sigma=sigma)
                loop.set_noise(noise)
                t = timed(lambda: loop.run_steps(args.steps), dev)
                finite = finite and bool(torch.isfinite(loop.latent).all())
                if i:
                    times[name].append(t / args.steps)
                    graphs.add((name[:3], id(loop.graph)))
        res = {k: {"ms_per_step": round(statistics.median(v), 4), "min_max": [round(min(v), 4), round(max(v), 4)]} for k, v in times.items()}
        for name in ("seg_inf_3b", "seg_10_3b"):
            res[name]["per_site_us"] = round((res[name]["ms_per_step"] - res["plain_3b"]["ms_per_step"]) * 1e3 / sites, 2)
        grid = seg.site_grid((latent, latent), (latent // 4) ** 2)
        blur, att = kernels_alone(dev, args.reps, grid, (spec.widths[-1] // spec.head_dim))
    line = json.dumps({"tool": "seg_time", "spec": args.spec, "dtype": "bf16", "latent": latent, "steps": args.steps, "runs": args.runs,
                       "seg_sites": sites, "finite": finite, "one_graph_for_both_sigmas": len([g for g in graphs if g[0] == "seg"]) == 1,
                       "loops": res, "blur": blur, "attention": att})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
