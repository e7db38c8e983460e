"""Write tests/golden/f1_unet_step_latent64_freeu.npz: one SDXL-base step at latent 64 with FreeU, on the CPU.

    python tools/make_freeu_golden.py [--no-f64]

The inputs are those of the F1 fixture (synthetic weights seed 0, synth.denoise_inputs(1, 64, 1234), timestep 999); FreeU is
version 1 at the SDXL values (s1 0.9, s2 0.2, b1 1.3, b2 1.4).  The network is the eager fp32 module of
stabletriton_amd/unet.py; FreeU is applied by the tests' own hook route (tests/freeu_util.py: forward_pre_hooks on the
decoder resnets, the published FFT filter in float64) - nothing of stabletriton_amd/freeu.py runs here.  Unless --no-f64
the same step is then run in float64 (20 GB of weights) and the fp32 output's largest deviation from it is recorded in
the file as `f64_max_abs_dev`, with `plain_max_abs_diff`: how far FreeU moves the output of the plain fp32 step.
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
from tests.freeu_util import SDXL_VALUES, hooked  # noqa: E402

NAME = "f1_unet_step_latent64_freeu"


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-f64", action="store_true")
    args = ap.parse_args()
    m = UNet2DConditionModel(SDXL_BASE).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    x = synth.denoise_inputs(1, 64, 1234)
    t = torch.tensor(999.0)

    def step(mod, cast):
        xi = {k: v.to(cast) for k, v in x.items()}
        return mod(xi["latent"], t, xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]

    plain = step(m, torch.float32)
    with hooked(m, **SDXL_VALUES, version=1):
        out = step(m, torch.float32)
    arrays = dict(out=out.numpy(), timestep=999.0, latent_hw=64, version=1, plain_max_abs_diff=float((out - plain).abs().max()),
                  **{k: np.asarray(v) for k, v in SDXL_VALUES.items()})
    print(f"|out| max {float(out.abs().max()):.4f}; FreeU moves the plain step by {arrays['plain_max_abs_diff']:.4f}")
    if not args.no_f64:
        m = m.double()
        with hooked(m, **SDXL_VALUES, version=1):
            out64 = step(m, torch.float64)
        arrays["f64_max_abs_dev"] = float((out.double() - out64).abs().max())
        print(f"fp32 eager vs float64: max abs deviation {arrays['f64_max_abs_dev']:.3e}")
    arrays.update(meta_torch_version=torch.__version__, meta_weight_seed=0, meta_input_seed=1234)
    path = os.path.join(ROOT, "tests", "golden", NAME + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
