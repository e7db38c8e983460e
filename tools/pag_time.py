"""What perturbed-attention guidance costs per step on SDXL-base bf16 at latent 128 (1024 x 1024 px), Euler 50: four captured
loops over one module compiled with pag_layers=("mid",), same weights, alternated in one process; then the identity kernel
alone and the three-way update kernels against their two-way counterparts.

    python tools/pag_time.py [--spec sdxl|tiny] [--steps 50] [--runs 5] [--out pag_time.json]

One JSON object.  "loops", milliseconds per step (one replay of the loop graph, host clock around a device synchronise, after one
warm-up replay of each; medians over --runs, with min and max):
  cfg_pag_3b     CFG + PAG: rows [negative | positive | perturbed], the ten mid-block self-attentions of the perturbed row are copies
  cfg_2b         CFG alone, 2B rows: the loop as it was
  plain_3b       the 3B loop with chunks = 0: the same rows, no perturbation (every attention runs)
  pag0_3b        pag_scale = 0 at 3B (the table is data: expected to equal cfg_pag_3b)
cfg_pag_3b against plain_3b is what skipping the ten attentions of one row buys, net of ten copy launches; plain_3b against cfg_2b
is the price of the third row block.
"identity": the identity kernel alone at (B, T, H, D) = (3, 1024, 20, 64) bf16, every entry perturbed, v the third column block
of a fused q|k|v buffer: microseconds per call (device events around `--reps` back-to-back calls) against its traffic floor, the
bytes read plus the bytes written at 6.3 TB/s.  The buffers are small enough to stay in the caches between calls: a lower bound of
what the kernel takes behind a q|k|v GEMM, not an HBM measurement.
"updates": the six update entry points at batch 1, latent 128, bf16: microseconds per call, three-way and two-way.
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
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_discrete_tables  # noqa: E402
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s
G, S = 5.0, 3.0


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


def identity_alone(dev, reps):
    B, T, H, D = 3, 1024, 20, 64
    C = H * D
    qkv = torch.randn((B, T, 3 * C), device=dev, dtype=torch.bfloat16)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    us = event_us(lambda: ops.attention_pag(q, k, v, H, D ** -0.5, B), reps, dev)
    full = event_us(lambda: ops.attention(q, k, v, H, D ** -0.5), reps, dev)
    nbytes = 2 * B * T * C * 2
    return {"shape": [B, T, H, D], "dtype": "bf16", "us_per_call": round(us, 2), "bytes": nbytes,
            "floor_us": round(nbytes / HBM_ACHIEVABLE * 1e6, 2), "attention_us_per_call": round(full, 2)}


def updates(dev, latent, reps):
    dt, cl = torch.bfloat16, torch.channels_last
    lat = torch.randn((1, 4, latent, latent), device=dev).contiguous(memory_format=cl)
    hist = torch.randn_like(lat)
    eps = {r: torch.randn((r, 4, latent, latent), device=dev, dtype=dt).contiguous(memory_format=cl) for r in (2, 3)}
    nxt = {r: torch.empty_like(eps[r]) for r in (2, 3)}
    step = torch.tensor([7], dtype=torch.int32, device=dev)
    start = torch.zeros(1, dtype=torch.int32, device=dev)
    seeds = torch.tensor([1234], dtype=torch.int64, device=dev)
    te, td, ts = euler_discrete_tables(50), dpmpp_2m_tables(50, karras=True), dpmpp_2m_sde_tables(50, karras=True)
    n = 50
    dsigma, in_scale = torch.tensor(te.dsigma(), device=dev), torch.tensor(te.in_scale(), device=dev)
    cd, cs = torch.tensor(td.coefficients(), device=dev), torch.tensor(ts.coefficients(), device=dev)
    g, s, phi = (torch.full((n,), v, device=dev) for v in (G, S, 0.7))
    ws = ops.cfg_workspace(lat)
    out = {}
    for name, resc in (("", None), ("_rescale", phi)):
        out["euler" + name] = {
            "two_way_us": event_us(lambda: ops.cfg_euler_step(lat, eps[2], nxt[2], dsigma, in_scale, g, step, resc, ws), reps, dev),
            "three_way_us": event_us(lambda: ops.pag_euler_step(lat, eps[3], nxt[3], dsigma, in_scale, g, s, step, resc, ws), reps, dev)}
        out["dpmpp2m" + name] = {
            "two_way_us": event_us(lambda: ops.dpmpp2m_step(lat, eps[2], nxt[2], hist, cd, in_scale, step, start, g, resc, ws), reps, dev),
            "three_way_us": event_us(lambda: ops.pag_dpmpp2m_step(lat, eps[3], nxt[3], hist, cd, in_scale, step, start, s, g, resc, ws), reps, dev)}
        out["sde" + name] = {
            "two_way_us": event_us(lambda: ops.sde_step(lat, eps[2], nxt[2], hist, cs, in_scale, step, start, seeds, g, resc, ws), reps, dev),
            "three_way_us": event_us(lambda: ops.pag_sde_step(lat, eps[3], nxt[3], hist, cs, in_scale, step, start, seeds, s, g, resc, ws), reps, dev)}
    return {k: {kk: round(vv, 2) for kk, vv in v.items()} for k, v in out.items()}


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
    m = build(spec, dt, dev)
    x = synth.denoise_inputs(2, latent, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    noise = x["latent"][:1]
    gm = optimize_model(m, cuda_graph=False, pag_layers=("mid",))
    with torch.no_grad():
        loops = {"cfg_pag_3b": make_loop(gm, spec, latent, dt, dev, args.steps, x, pag_scale=S),
                 "cfg_2b": make_loop(gm, spec, latent, dt, dev, args.steps, x),
                 "plain_3b": make_loop(gm, spec, latent, dt, dev, args.steps, x, pag_scale=S),
                 "pag0_3b": make_loop(gm, spec, latent, dt, dev, args.steps, x, pag_scale=0.0)}
        loops["plain_3b"]._perturbed_chunks = 0    # the same 3B rows and update, every attention ordinary (set before its capture)
        times = {k: [] for k in loops}
        finite = True
        for i in range(args.runs + 1):                             # (round 0 captures and warms every graph up)
            for name, loop in loops.items():
                loop.set_noise(noise)
                t = timed(lambda: loop.run_steps(args.steps), dev)
                finite = finite and bool(torch.isfinite(loop.latent).all())
                if i:
                    times[name].append(t / args.steps)
        res = {k: {"ms_per_step": round(statistics.median(v), 4), "min_max": [round(min(v), 4), round(max(v), 4)]} for k, v in times.items()}
        ident = identity_alone(dev, args.reps)
        upd = updates(dev, latent, args.reps)
    line = json.dumps({"tool": "pag_time", "spec": args.spec, "dtype": "bf16", "latent": latent, "steps": args.steps, "runs": args.runs,
                       "pag_sites": gm.rewrite_stats["pag_sites"], "finite": finite, "loops": res, "identity": ident, "updates": upd})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
