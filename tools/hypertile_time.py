"""What one windowed self-attention launch costs (HyperTile, csrc/attention_windows.hip) beside `st_attention` at the same shape, in one
process on one device: bf16, B = 2, 10 heads of 64, T = 4096 (64 x 64 grid) and T = 16,384 (128 x 128), tilings (1, 1), (2, 2), (4, 4),
every tiling at the query rows per block a loop's site would fix (hypertile.rows_per_block) and, as `..._r128`, at 128 rows (four
waves and a loader), the other form that divides every window here.

    python tools/hypertile_time.py [--rounds 7] [--out profiles/hypertile_time.json]

Each figure is device time per launch inside a replayed graph of n launches (device events around as many replays as make the timed
window about WINDOW_MS long: kernel and its boundary in a graph, as the loop runs it, without the host's launch path).  The graphs of
one shape are timed in turn, attention, (1, 1), (2, 2), (4, 4), attention ..., after one warm-up round; medians over --rounds with min and max.  `one_one_inside_attention_range` says
whether the (1, 1) median lies inside [min, max] of `st_attention` measured beside it.  Not measured: other head counts and batches, fp16,
the loop end to end, windows whose width is no power of two."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from stabletriton_amd import hypertile, ops, synth  # noqa: E402

B, H, D = 2, 10, 64
TILINGS = ((1, 1), (2, 2), (4, 4))
WINDOW_MS = 30.0


def graph_of(fn, n, dev):
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


def replay_us(g, n, dev, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / (n * reps) * 1e3


def shape(side, rounds, dev):
    T, C = side * side, H * D
    qkv = synth.normal(f"hypertile.qkv{side}", (B, T, 3 * C), 11, dev).to(torch.bfloat16)      # the fused projection's buffer: column slices
    q, k, v = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
    rows = hypertile.rows_per_block(T, H, B)
    n = 40 if T <= 4096 else 10
    scale = D ** -0.5
    graphs = {"attention": graph_of(lambda: ops.attention(q, k, v, H, scale), n, dev)}
    for r, tag in ((rows, ""), (128, "_r128")):
        for t in TILINGS:
            graphs[f"windows_{t[0]}x{t[1]}{tag}"] = graph_of(lambda t=t, r=r: ops.attention_windows(q, k, v, H, scale, (side, side), tiling=t, rows=r,
                                                                                                  fused=True), n, dev)
    same = bool(torch.equal(ops.attention(q, k, v, H, scale), ops.attention_windows(q, k, v, H, scale, (side, side), tiling=(1, 1), rows=rows)))
    times = {name: [] for name in graphs}
    reps = {name: max(1, round(WINDOW_MS * 1e3 / (replay_us(g, n, dev) * n))) for name, g in graphs.items()}
    for i in range(rounds + 1):                                    # (round 0 warms up)
        for name, g in graphs.items():
            us = replay_us(g, n, dev, reps[name])
            if i:
                times[name].append(us)
    med = {k_: statistics.median(v_) for k_, v_ in times.items()}
    lo, hi = min(times["attention"]), max(times["attention"])
    return {"tokens": T, "grid": [side, side], "rows_per_block": rows, "launches_per_graph": n, "window_ms": WINDOW_MS,
            **{f"{k_}_us": round(med[k_], 2) for k_ in times},
            **{f"{k_}_min_max": [round(min(v_), 2), round(max(v_), 2)] for k_, v_ in times.items()},
            "one_one_inside_attention_range": bool(lo <= med["windows_1x1"] <= hi), "one_one_is_attention_bit_for_bit": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with torch.no_grad():
        line = json.dumps({"tool": "hypertile_time", "dtype": "bf16", "batch": B, "heads": H, "head_dim": D, "rounds": args.rounds,
                           "shapes": [shape(side, args.rounds, dev) for side in (64, 128)]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
