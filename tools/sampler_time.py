"""Euler at 50 steps against DPM-Solver++(2M) with Karras sigmas at 25 steps, and the stochastic samplers at the same step
counts (Euler ancestral at 50, DPM++ 2M SDE Karras at 25), SDXL-base 1024 px (latent 128), bs=1, bf16, mode loop, one
process: ms per image, without and with classifier-free guidance 5.0.

    python tools/sampler_time.py [--runs 5] [--euler-steps 50] [--dpm-steps 25] [--out sampler_time.json]

All four loops run over the same compiled module.  Whole trajectories (one graph launch each) are timed alternately,
A B A B ..., after one warm-up trajectory of each, host clock around a device synchronise.  A second part times the update
ops alone at the loops' shapes: 200 calls captured in one graph per op, so the per-call figure carries no host launch cost
(`euler_step`, `cfg_euler_step`, `dpmpp2m_step` and `sde_step` plain and guided; `sde_step` on a row that draws noise).  Prints one JSON line.
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
from stabletriton_amd.scheduler import (dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_ancestral_tables,  # noqa: E402
                                        euler_discrete_tables)
from stabletriton_amd.unet import SDXL_BASE, UNet2DConditionModel  # noqa: E402
from tools.cfg_loop_time import graph_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--euler-steps", type=int, default=50)
    ap.add_argument("--dpm-steps", type=int, default=25)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    with torch.device("meta"):
        m = UNet2DConditionModel(SDXL_BASE)
    m = m.to_empty(device=dev).to(dt).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    gm = optimize_model(m, cuda_graph=False)
    eu_t = euler_discrete_tables(args.euler_steps)
    dpm_t = dpmpp_2m_tables(args.dpm_steps, karras=True)
    eua_t = euler_ancestral_tables(args.euler_steps)
    sde_t = dpmpp_2m_sde_tables(args.dpm_steps, karras=True)
    x = synth.denoise_inputs(2, args.latent, 1234, device=dev)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    loops = {}
    for name, tables in ((f"euler{args.euler_steps}", eu_t), (f"dpmpp2m_karras{args.dpm_steps}", dpm_t),
                         (f"euler_a{args.euler_steps}", eua_t), (f"dpmpp2m_sde_karras{args.dpm_steps}", sde_t)):
        plain = DenoiseLoop(gm, 1, args.latent, dt, dev, tables, mode="loop")
        plain.set_conditioning(*(c[1:2] for c in cond))
        guided = DenoiseLoop(gm, 1, args.latent, dt, dev, tables, mode="loop", guidance_scale=5.0)
        guided.set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
        loops[name] = plain
        loops[name + "_cfg5"] = guided
    noise = x["latent"][:1]
    times = {k: [] for k in loops}
    with torch.no_grad():
        for lp in loops.values():
            lp.capture()
            lp.denoise(noise, seed=1234)                           # warm-up trajectory (the seed drives the SDE noise)
        for _ in range(args.runs):
            for k, lp in loops.items():
                lp.set_noise(noise)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                lp.run_steps(lp.n_steps)
                torch.cuda.synchronize(dev)
                times[k].append((time.perf_counter() - t0) * 1e3)
        finite = all(bool(torch.isfinite(lp.latent).all()) for lp in loops.values())

        # the update ops alone, at the loops' shapes (bs=1 latent; guided eps / next_in at 2 rows)
        e_plain, e_cfg = loops[f"euler{args.euler_steps}"], loops[f"euler{args.euler_steps}_cfg5"]
        d_plain, d_cfg = loops[f"dpmpp2m_karras{args.dpm_steps}"], loops[f"dpmpp2m_karras{args.dpm_steps}_cfg5"]
        s_plain, s_cfg = loops[f"dpmpp2m_sde_karras{args.dpm_steps}"], loops[f"dpmpp2m_sde_karras{args.dpm_steps}_cfg5"]
        assert float(s_plain.coef[10, 4]) != 0.0                   # the timed row draws noise
        lat = e_plain.latent.clone()
        eps1, eps2 = torch.randn_like(e_plain.x_in), torch.randn_like(e_cfg.x_in)
        nxt1, nxt2 = torch.empty_like(e_plain.x_in), torch.empty_like(e_cfg.x_in)
        hist = torch.zeros_like(lat)
        ids, dids = e_plain.step_ids[10:11], d_plain.step_ids[10:11]
        op_us = {
            "euler_step_b1": graph_us(lambda: ops.euler_step(lat, eps1, nxt1, e_plain.dsigma, e_plain.in_scale, ids)),
            "cfg_euler_step_b1": graph_us(lambda: ops.cfg_euler_step(lat, eps2, nxt2, e_cfg.dsigma, e_cfg.in_scale, e_cfg.guidance,
                                                                     ids)),
            "dpmpp2m_step_b1": graph_us(lambda: ops.dpmpp2m_step(lat, eps1, nxt1, hist, d_plain.coef, d_plain.in_scale, dids,
                                                                 d_plain.start)),
            "dpmpp2m_step_cfg_b1": graph_us(lambda: ops.dpmpp2m_step(lat, eps2, nxt2, hist, d_cfg.coef, d_cfg.in_scale, dids,
                                                                     d_cfg.start, guidance=d_cfg.guidance)),
            "sde_step_b1": graph_us(lambda: ops.sde_step(lat, eps1, nxt1, hist, s_plain.coef, s_plain.in_scale, dids, s_plain.start,
                                                         s_plain.seeds)),
            "sde_step_cfg_b1": graph_us(lambda: ops.sde_step(lat, eps2, nxt2, hist, s_cfg.coef, s_cfg.in_scale, dids, s_cfg.start,
                                                             s_cfg.seeds, guidance=s_cfg.guidance)),
        }

    med = {k: statistics.median(v) for k, v in times.items()}
    eu, dp = f"euler{args.euler_steps}", f"dpmpp2m_karras{args.dpm_steps}"
    ea, sd = f"euler_a{args.euler_steps}", f"dpmpp2m_sde_karras{args.dpm_steps}"
    res = {"what": f"SDXL-base {args.latent * 8} px bf16 bs=1, mode loop: Euler {args.euler_steps} steps vs DPM++(2M) Karras "
                   f"{args.dpm_steps} steps, and their stochastic counterparts (Euler ancestral, DPM++ 2M SDE Karras), "
                   f"without / with CFG 5, same process, alternating",
           "ms_per_image_median": {k: round(v, 2) for k, v in med.items()},
           "ms_per_image_all": {k: [round(t, 2) for t in v] for k, v in times.items()},
           "dpm_over_euler_time": {"plain": round(med[dp] / med[eu], 3), "cfg5": round(med[dp + "_cfg5"] / med[eu + "_cfg5"], 3)},
           "stochastic_over_deterministic_time": {"euler_a_over_euler": round(med[ea] / med[eu], 3),
                                                  "euler_a_over_euler_cfg5": round(med[ea + "_cfg5"] / med[eu + "_cfg5"], 3),
                                                  "sde_over_dpmpp2m": round(med[sd] / med[dp], 3),
                                                  "sde_over_dpmpp2m_cfg5": round(med[sd + "_cfg5"] / med[dp + "_cfg5"], 3)},
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
