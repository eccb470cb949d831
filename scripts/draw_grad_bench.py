"""Micro-timing of the gradient of the layered rasteriser (render.draw_with_grad: dsvg_raster_sweep_layers_nn forward,
dsvg_raster_blend_bwd + dsvg_raster_sweep_layers_bwd + dsvg_raster_segments_layers_bwd backward) in one process, on 512 icons of
synthetic.make_batch (float32 arguments) at 64 and 128 pixels per side:
  (a) the forward twin against render.draw, every group FILL and mixed modes: the twin writes 8 bytes more per pixel and layer
      (the coverage and the arg-min);
  (b) forward + backward of draw_with_grad, every group FILL and mixed modes, the gradient taken with respect to the
      arguments, the colours and the opacities;
  (c) the workaround there was before, for the all-FILL case only (the only one it can express): G flattened
      rasterize_with_grad(fill=True) images and the torch compositing line of rasterize's docstring, forward + backward.  Its
      composite is the maximum-ink one, not draw's blend, and it has no gradient for an opacity.
The variants alternate inside every round; a time is the median over the rounds of the mean of `reps` calls between two device
events, the spread is the range over the rounds.  Prints the times and the ratios and writes them to --log (default
profiles/draw_grad_bench.log, appended to when --append is given)."""
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
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "draw_grad_bench.log"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--icons", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("draw_grad_bench: needs a GPU (a CPU run measures nothing)")
    commands, args = (t.to("cuda") for t in make_batch(a.icons, seed=3))
    commands, args = commands.float(), args.float()
    N, G, S = commands.shape
    all_fill = torch.ones(N, G, dtype=torch.int64, device="cuda")
    mixed = (torch.arange(G, device="cuda") % 3).expand(N, G).contiguous()
    flat_c = commands.reshape(N * G, S)
    leaf = args.clone().requires_grad_(True)
    colors = render.palette(G, device="cuda").requires_grad_(True)
    opacity = torch.full((G,), 0.75, device="cuda", requires_grad=True)
    lines = [f"{torch.cuda.get_device_name(0)}; {N} icons of make_batch, G={G}, S={S}, n=10, float32 arguments; microseconds per "
             f"call: median of {a.rounds} rounds (variants alternating), each the mean of {a.reps} calls; [min .. max] over the rounds"]
    for size in (64, 128):
        dout = torch.rand(N, 3, size, size, device="cuda")

        def twin(filling):
            with torch.no_grad():
                return render.draw_with_grad(commands, args, filling=filling, colors=colors, opacity=opacity, size=size)

        def both(filling):
            leaf.grad = colors.grad = opacity.grad = None
            render.draw_with_grad(commands, leaf, filling=filling, colors=colors, opacity=opacity, size=size).backward(dout)

        def composed():
            leaf.grad = colors.grad = None
            layers = render.rasterize_with_grad(flat_c, leaf.reshape(N * G, S, 11), size=size, fill=True).view(N, G, 1, size, size)
            (1 - (layers * (1 - colors).view(1, G, 3, 1, 1)).amax(1)).backward(dout)

        detached = (colors.detach(), opacity.detach())
        variants = {
            "draw_fill": lambda: render.draw(commands, args, filling=all_fill, colors=detached[0], opacity=detached[1], size=size),
            "twin_fill": lambda: twin(all_fill),
            "draw_mixed": lambda: render.draw(commands, args, filling=mixed, colors=detached[0], opacity=detached[1], size=size),
            "twin_mixed": lambda: twin(mixed),
            "fwd_bwd_fill": lambda: both(all_fill),
            "fwd_bwd_mixed": lambda: both(mixed),
            "groups_composed_fwd_bwd": composed,
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
        extra = 8 * N * G * size * size
        lines.append(f"size {size}: (a) the twin takes {med['twin_fill'] / med['draw_fill']:.2f}x the time of draw all-FILL, "
                     f"{med['twin_mixed'] / med['draw_mixed']:.2f}x mixed ({extra / 1e6:.1f} MB more written, {med['twin_fill'] - med['draw_fill']:+.1f} "
                     f"us all-FILL); (b) forward "
                     f"+ backward {med['fwd_bwd_fill'] / med['draw_fill']:.2f}x of draw all-FILL, {med['fwd_bwd_mixed'] / med['draw_mixed']:.2f}x "
                     f"mixed; (c) G images + torch compositing, forward + backward, takes "
                     f"{med['groups_composed_fwd_bwd'] / med['fwd_bwd_fill']:.2f}x the time of (b) all-FILL")
        both(mixed)
        lines.append(f"size {size}: mixed modes: max |d args| {leaf.grad.abs().max().item():.3e}, max |d colours| "
                     f"{colors.grad.abs().max().item():.3e}, max |d opacity| {opacity.grad.abs().max().item():.3e}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "a" if a.append else "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
