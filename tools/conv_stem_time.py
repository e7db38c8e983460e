"""What the nine-channel stem costs next to the four-channel one, at SDXL's conv_in size (128 x 128, Cout = 320, bf16), N = 1 and 2, in
one process on one device:

  (a) st_conv_stem, two sources: the loop's 4-channel x_in plus the 5-channel condition of one image;
  (b) st_conv_stem on one 9-channel tensor (18-byte pixels: element loads);
  (c) the thin kernel (st_conv2d) on the 4-channel conv_in of the same size - the existing stem, the thing to measure against;
  (d) a device-to-device copy of the output's bytes - the write floor.

    python tools/conv_stem_time.py [--launches 300] [--replays 7] [--out profiles/conv_stem_time.json]

tools/inpaint_time.py's method: device events around one replay of a captured graph of --launches launches of the one kernel (kernel
boundaries included, the host's launch path not), median over --replays with min and max, per launch in microseconds."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from stabletriton_amd import ops, synth  # noqa: E402


def graph_us(fn, dev, n, replays):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize(dev)
        out.append(a.elapsed_time(b) / n * 1e3)
    return {"median_us": round(statistics.median(out), 3), "min_max_us": [round(min(out), 3), round(max(out), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--replays", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, dt, cl = torch.device("cuda:0"), torch.bfloat16, torch.channels_last
    side, cout = 128, 320
    res = {"tool": "conv_stem_time", "dtype": "bf16", "latent": side, "cout": cout, "launches": args.launches, "replays": args.replays}
    w9 = (synth.normal("stem.w9", (cout, 9, 3, 3), 1, dev) / 9).to(dt).contiguous(memory_format=cl)
    w4 = (synth.normal("stem.w4", (cout, 4, 3, 3), 2, dev) / 6).to(dt).contiguous(memory_format=cl)
    bias = synth.normal("stem.b", (cout,), 3, dev).to(dt)
    with torch.no_grad():
        for n in (1, 2):
            x4 = synth.normal("stem.x", (n, 4, side, side), 4, dev).to(dt).contiguous(memory_format=cl)
            cond = synth.normal("stem.c", (1, 5, side, side), 5, dev).to(dt).contiguous(memory_format=cl)
            x9 = torch.cat([x4, cond.expand(n, -1, -1, -1)], dim=1).contiguous(memory_format=cl)
            two, one = ops.conv_stem(x4, cond, w9, bias), ops.conv_stem(x9, None, w9, bias)
            dst = torch.empty_like(two)
            res[f"n{n}"] = {
                "stem_two_sources": graph_us(lambda: ops.conv_stem(x4, cond, w9, bias), dev, args.launches, args.replays),
                "stem_one_tensor": graph_us(lambda: ops.conv_stem(x9, None, w9, bias), dev, args.launches, args.replays),
                "thin_four_channels": graph_us(lambda: ops.conv2d(x4, w4, bias, 1, 1), dev, args.launches, args.replays),
                "copy_output_bytes": graph_us(lambda: dst.copy_(two), dev, args.launches, args.replays),
                "output_bytes": two.numel() * two.element_size(),
                "forms_agree_bit_for_bit": bool(torch.equal(two, one)), "finite": bool(torch.isfinite(two).all())}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
