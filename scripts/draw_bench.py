"""Micro-timing of the layered rasteriser (render.draw: dsvg_raster_segments_layers + dsvg_raster_sweep_layers) in one process,
on 512 icons of synthetic.make_batch at 64 and 128 pixels per side:
  (a) draw with every group FILL, and with mixed modes (outline / fill / erase by group), colours from render.palette;
  (b) rasterize(fill=True) on the same batch: the existing kernel, the same crossing work per pixel and chord, one channel -
      the floor;
  (c) what there was before draw: rasterize(fill=True) on the flattened [N * G, S] groups and the torch compositing line of
      rasterize's docstring (G one-channel images, then several torch launches over them).  It cannot draw an erase path.
The variants alternate inside every round; a time is the median over the rounds of the mean of `reps` calls between two device
events, the spread is the range over the rounds.  Prints the times and the ratios (a) / (b) and (c) / (a) and writes them to
--log (default profiles/draw_bench.log)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepsvg_amd import render       # noqa: E402
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
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "draw_bench.log"))
    ap.add_argument("--icons", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("draw_bench: needs a GPU (a CPU run measures nothing)")
    commands, args = (t.to("cuda") for t in make_batch(a.icons, seed=3))
    N, G, S = commands.shape
    colors = render.palette(G, device="cuda")
    all_fill = torch.ones(N, G, dtype=torch.int64, device="cuda")
    mixed = (torch.arange(G, device="cuda") % 3).expand(N, G).contiguous()
    flat_c, flat_a = commands.reshape(N * G, S), args.reshape(N * G, S, 11)
    ink = (1 - colors).view(1, G, 3, 1, 1)
    lines = [f"{torch.cuda.get_device_name(0)}; {N} icons of make_batch, G={G}, S={S}, n=10; microseconds per call: median of "
             f"{a.rounds} rounds (variants alternating), each the mean of {a.reps} calls; [min .. max] over the rounds"]
    for size in (64, 128):
        def composed():
            layers = render.rasterize(flat_c, flat_a, size=size, fill=True).view(N, G, 1, size, size)
            return 1 - (layers * ink).amax(1)
        variants = {
            "draw_fill": lambda: render.draw(commands, args, filling=all_fill, colors=colors, size=size),
            "draw_mixed": lambda: render.draw(commands, args, filling=mixed, colors=colors, size=size),
            "rasterize_fill": lambda: render.rasterize(commands, args, size=size, fill=True),
            "groups_composed": composed,
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
            lines.append(f"size {size} {k}: {med[k]:.1f} us [{min(v):.1f} .. {max(v):.1f}]")
        lines.append(f"size {size}: (a) / (b): draw all-FILL {med['draw_fill'] / med['rasterize_fill']:.2f}x, draw mixed "
                     f"{med['draw_mixed'] / med['rasterize_fill']:.2f}x of rasterize(fill=True); (c) / (a): G images + torch "
                     f"compositing takes {med['groups_composed'] / med['draw_fill']:.2f}x the time of draw all-FILL")
        # the two ways to colour filled groups agree where the groups do not overlap; the pictures are not empty
        picture = variants["draw_fill"]()
        lines.append(f"size {size}: mean of the all-FILL picture {picture.mean().item():.4f}, of the composed one "
                     f"{composed().mean().item():.4f}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
