"""Write tests/golden/f1_unet_step_latent64_seg.npz: one SDXL-base step at latent 64 with smoothed-energy attention, on the CPU.

    python tools/make_seg_golden.py [--no-f64] [--layers down_blocks mid up_blocks]

Three UNet rows [negative | positive | perturbed] as DenoiseLoop(guidance_scale=..., seg_scale=...) lays them out: synthetic
weights seed 0; tests/pag_util.three_rows: synth.denoise_inputs(2, 64, 1234) gives the negative prompt (row 0), the prompt (row 1)
and the latent (row 0, the same in all three rows); the perturbed row carries the prompt; timestep 999; sigma = infinity (the queries'
spatial mean); sites ("down_blocks", "mid", "up_blocks") = all seventy self-attentions (32 x 32 and 16 x 16 token grids).  At this
timestep the perturbed row is 8.5e-3 from the positive one with ("mid",) alone and 5.1e-2 with ("down_blocks.2", "mid"): too little
for a check at the 1e-3 gate to tell a working perturbation from a broken one with two orders of magnitude to spare; with every
self-attention it is 0.157, recorded in the file.  The network is the eager
fp32 module of stabletriton_amd/unet.py; the perturbation is applied by the tests' own hook route (tests/seg_util.py: forward hooks
that recompute the tail rows of attn1's output with float64-blurred queries) - nothing of stabletriton_amd/seg.py runs here.  Only
the output rows are stored.  Unless --no-f64 the same step is then run in float64 (20 GB of weights) and the fp32 output's largest
deviation from it is recorded as `f64_max_abs_dev`; `pert_vs_pos_max_abs` is how far the perturbed row's prediction is from the
positive one.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stabletriton_amd import synth  # noqa: E402
from stabletriton_amd.unet import SDXL_BASE, UNet2DConditionModel  # noqa: E402
from tests.pag_util import selected, three_rows  # noqa: E402
from tests.seg_util import hooked  # noqa: E402

NAME = "f1_unet_step_latent64_seg"
SIGMA = float("inf")
HW = 64


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-f64", action="store_true")
    ap.add_argument("--layers", nargs="+", default=["down_blocks", "mid", "up_blocks"])
    args = ap.parse_args()
    layers = tuple(args.layers)
    m = UNet2DConditionModel(SDXL_BASE).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    sites = selected(m, layers)
    x = three_rows(HW, 1234)
    t = torch.tensor(999.0)

    def step(mod, cast):
        xi = {k: v.to(cast) for k, v in x.items()}
        with hooked(mod, layers, 3, (HW, HW), SIGMA):
            return mod(xi["latent"], t, xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]

    out = step(m, torch.float32)
    gap = float((out[2] - out[1]).abs().max())
    arrays = dict(out=out.numpy(), timestep=999.0, latent_hw=HW, chunks=3, sites=len(sites), sigma=SIGMA, layers=np.array(layers),
                  pert_vs_pos_max_abs=gap)
    print(f"|out| max {float(out.abs().max()):.4f}; the perturbed row is {gap:.4f} from the positive one ({len(sites)} sites)")
    if not args.no_f64:
        m = m.double()
        out64 = step(m, torch.float64)
        arrays["f64_max_abs_dev"] = float((out.double() - out64).abs().max())
        print(f"fp32 eager vs float64: max abs deviation {arrays['f64_max_abs_dev']:.3e}")
    arrays.update(meta_torch_version=torch.__version__, meta_weight_seed=0, meta_input_seed=1234)
    path = os.path.join(ROOT, "tests", "golden", NAME + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
