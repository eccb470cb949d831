"""Micro-timing of the filling of a decoded batch (paths.compute_filling: dsvg_raster_segments_layers + dsvg_overlap_counts +
dsvg_filling_from_counts) in one process, on 512 icons of synthetic.make_batch at 64 and 128 samples per side:
  (a) overlap_counts alone, on records built once (the two zeroed count tables it adds into are part of the call);
  (b) raster_sweep(fill=True, size=samples) alone, on records built once: the fill sweep, the same crossing work per sample
      and chord plus the distance work - the yardstick (csrc/raster.hip compiles to the parent commit's code);
  (c) the whole compute_filling (three launches) and the whole overlap (two launches and the fraction);
  (d) the whole rasterize(fill=True, size=samples) (two launches).
The variants alternate inside every round; a time is the median over the rounds of the mean of `reps` calls between two device
events, the spread is the range over the rounds.  Prints the times and the ratios (a) / (b) and (c) / (d) and writes them to
--log (default profiles/filling_bench.log)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepsvg_amd import ops, paths, render       # noqa: E402
from deepsvg_amd.synthetic import make_batch       # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "filling_bench.log"))
    ap.add_argument("--icons", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filling_bench: needs a GPU (a CPU run measures nothing)")
    commands, args = (t.to("cuda") for t in make_batch(a.icons, seed=3))
    N, G, S = commands.shape
    flat_c, flat_a = commands.reshape(N * G, S).contiguous(), args.reshape(N * G, S, 11).contiguous()
    modes = torch.ones(N, G, dtype=torch.int32, device="cuda")
    layered = ops.raster_segments_layers(flat_c, flat_a, modes, n=10, groups=G)
    filled = ops.raster_segments(flat_c, flat_a, n=10, groups=G, fill=True)
    lines = [f"{torch.cuda.get_device_name(0)}; {N} icons of make_batch, G={G}, S={S}, n=10, "
             f"{int(layered[1].sum())} chord records; microseconds per call: median of {a.rounds} rounds (variants alternating), "
             f"each the mean of {a.reps} calls; [min .. max] over the rounds"]
    for samples in (64, 128):
        variants = {
            "overlap_counts": lambda: ops.overlap_counts(*layered, samples=samples),
            "raster_sweep_fill": lambda: ops.raster_sweep(*filled, size=samples, fill=True),
            "compute_filling": lambda: paths.compute_filling(commands, args, samples=samples),
            "overlap": lambda: paths.overlap(commands, args, samples=samples),
            "rasterize_fill": lambda: render.rasterize(commands, args, size=samples, fill=True),
        }
        for fn in variants.values():          # code objects, allocator blocks
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn, a.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            lines.append(f"samples {samples} {k}: {med[k]:.1f} us [{min(v):.1f} .. {max(v):.1f}]")
        lines.append(f"samples {samples}: (a) / (b): overlap_counts takes {med['overlap_counts'] / med['raster_sweep_fill']:.2f}x the "
                     f"time of the fill sweep; (c) / (d): compute_filling {med['compute_filling'] / med['rasterize_fill']:.2f}x, "
                     f"overlap {med['overlap'] / med['rasterize_fill']:.2f}x of rasterize(fill=True)")
        # the counts agree with the picture: samples inside some group against pixels the fill sweep calls inside
        r = variants["compute_filling"]()
        ink = variants["rasterize_fill"]()
        lines.append(f"samples {samples}: samples inside a group, summed over groups {int(r['area'].sum())}; pixels with ink > 0.5 "
                     f"{int((ink > 0.5).sum())}; groups FILL {int((r['filling'] == 1).sum())}, ERASE {int((r['filling'] == 2).sum())}, "
                     f"left as outlines {int((r['filling'] == 0).sum())} of {N * G}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
