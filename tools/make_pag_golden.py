"""Write tests/golden/f1_unet_step_latent64_pag.npz: one SDXL-base step at latent 64 with perturbed attention, on the CPU.

    python tools/make_pag_golden.py [--no-f64]

Three UNet rows [negative | positive | perturbed] as DenoiseLoop(guidance_scale=..., pag_scale=...) lays them out: synthetic
weights seed 0; tests/pag_util.three_rows: synth.denoise_inputs(2, 64, 1234) gives the negative prompt (row 0), the prompt (row 1) and the latent (row 0,
the same in all three rows); the perturbed row carries the prompt; timestep 999; sites ("mid",) = the ten self-attentions of
the middle block.  The network is the eager fp32 module of stabletriton_amd/unet.py; the perturbation is applied by the tests'
own hook route (tests/pag_util.py: forward hooks that overwrite the tail rows of attn1's output with to_out(to_v(x))) - nothing of
stabletriton_amd/pag.py runs here.  Only the output rows are stored.  Unless --no-f64 the same step is then run in float64 (20 GB
of weights) and the fp32 output's largest deviation from it is recorded as `f64_max_abs_dev`; `pert_vs_pos_max_abs` is how far
the perturbed row's prediction is from the positive one.
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
from tests.pag_util import hooked, selected, three_rows  # noqa: E402

NAME = "f1_unet_step_latent64_pag"
LAYERS = ("mid",)


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-f64", action="store_true")
    args = ap.parse_args()
    m = UNet2DConditionModel(SDXL_BASE).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    sites = selected(m, LAYERS)
    assert len(sites) == 10, sites
    x = three_rows(64, 1234)
    t = torch.tensor(999.0)

    def step(mod, cast):
        xi = {k: v.to(cast) for k, v in x.items()}
        with hooked(mod, LAYERS, 3):
            return mod(xi["latent"], t, xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]

    out = step(m, torch.float32)
    gap = float((out[2] - out[1]).abs().max())
    arrays = dict(out=out.numpy(), timestep=999.0, latent_hw=64, chunks=3, sites=len(sites), pert_vs_pos_max_abs=gap)
    print(f"|out| max {float(out.abs().max()):.4f}; the perturbed row is {gap:.4f} from the positive one")
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
