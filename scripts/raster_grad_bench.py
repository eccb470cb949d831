"""Micro-timing of the gradient of the rasteriser (csrc/raster.hip) at batch 512, on the shapes and the batch of
scripts/raster_bench.py (G = 8 groups of S + 2 = 32 tokens, deepsvg_amd.synthetic's typical fill, n = 10), sizes 64 and 128,
stroke and fill:

  ops.raster_sweep_nn      next to ops.raster_sweep (both culled, the default): the two arms ALTERNATE inside one process, the
                           images are compared in bits.  The index costs two more vector instructions per pixel-chord pair
                           (compare + two selects in place of one minimum: 14 against 12 in stroke mode)
  ops.raster_sweep_bwd     16 lanes per chord next to a wave per chord, alternating; dout = 2 (image - target) / pixels
  ops.raster_segments_bwd
  one refine_to_images step  image_loss forward, backward, Adam
  the same definition as plain torch with autograd on the same GPU: a loop over icons of one [pixels, chords] fp32 broadcast
                           each, forward + backward with respect to the record vertices (counts on the host) - what one would
                           write without the kernels

HIP events around `inner` back-to-back calls, median [min .. max] of 20 such runs after warm-up (raster_bench.timed /
timed_ab).  Writes nothing but stdout."""
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raster_bench import G, N, NPTS, RUNS, S, timed, timed_ab          # noqa: E402
from deepsvg_amd import ops, render                  # noqa: E402
from deepsvg_amd.synthetic import make_batch         # noqa: E402


def torch_loop_grad(segs, counts, dout, size, stroke_width, fill):
    """the definition of include/dsvg.h one icon at a time with autograd: d sum(dout * image) / d (ax, ay, bx, by) -> [B, cap, 4].
    Written with the kernels' conventions, without which autograd returns NaN for whole icons (sqrt'(0) = inf at a pixel that
    sits on a chord, times the zeros of amin's mask - and integer arguments put vertices on pixel centres all the time): a
    pixel at d = 0 and a pixel whose ink is exactly 0 or 1 contribute nothing.  What is left to differ, and does on this batch
    of integer arguments: amin's backward splits a tie between the tied chords where the kernel gives it to the lowest index,
    and at a pixel whose centre lies on a chord up to rounding (an `l` through even coordinates passes through centres) d is
    ~1e-6 instead of 0 and the unit vector q / d is rounding noise, another one in every order of operations"""
    s = 256.0 / size
    centre = (torch.arange(size, device=segs.device, dtype=torch.float32) + 0.5) * s
    cx, cy = centre.view(1, 1, size), centre.view(1, size, 1)
    grad = torch.zeros(segs.shape[0], segs.shape[1], 4, device=segs.device)
    for i, k in enumerate(counts):
        if k == 0:
            continue
        r = segs[i, :k]
        v = torch.cat([r[:, :2], r[:, :2] + r[:, 2:4]], 1).requires_grad_(True)          # ax, ay, bx, by
        ax, ay, bx, by = (v[:, j].view(-1, 1, 1) for j in range(4))
        dx, dy = bx - ax, by - ay
        px, py = cx - ax, cy - ay
        len2 = dx * dx + dy * dy
        t = ((px * dx + py * dy) / len2.clamp(min=1e-30)).clamp(0, 1)
        d2 = ((px - t * dx) ** 2 + (py - t * dy) ** 2).amin(0)
        d = torch.where(d2 > 0, torch.where(d2 > 0, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
        if not fill:
            img = 0.5 + (stroke_width / 2 - d) / s
        else:
            with torch.no_grad():
                right = (ax + py * dx / torch.where(dy != 0, dy, torch.ones_like(dy))) > cx
                w = (((ay <= cy) & (cy < by) & right).to(torch.int32) - ((by <= cy) & (cy < ay) & right).to(torch.int32))
                seq = (r[:, 4].contiguous().view(torch.int32) & 1).long().cumsum(0) - 1
                wind = torch.zeros(int(seq[-1]) + 1, size, size, dtype=torch.int32, device=segs.device).index_add_(0, seq, w)
                inside = (wind != 0).any(0)
            img = torch.where(inside, 0.5 + d / s, 0.5 - d / s)
        img = torch.where((img > 0) & (img < 1), img, img.detach().clamp(0, 1))
        (img * dout[i]).sum().backward()
        grad[i, :k] = v.grad
    return grad


def main():
    assert torch.cuda.is_available(), "raster_grad_bench.py measures on a GPU"
    dev = "cuda"
    print(f"box {socket.gethostname()}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
    print(f"batch {N}, G = {G}, S + 2 = {S + 2}, n = {NPTS}, typical fill; median [min .. max] of {RUNS} runs")
    commands, args = make_batch(N, G=G, S=S, seed=1, device=dev)
    target_commands, target_args = make_batch(N, G=G, S=S, seed=2, device=dev)
    c, a = commands.reshape(N * G, S + 2).float().contiguous(), args.reshape(N * G, S + 2, 11).float().contiguous()
    for fill in (False, True):
        mode = "fill" if fill else "stroke"
        segs, counts = ops.raster_segments(c, a, n=NPTS, groups=G, fill=fill)
        total = int(counts.sum())
        host_counts = counts.tolist()
        print(f"[{mode}] {total} chords, mean {total / N:.0f} / max {int(counts.max())} per image, cap {segs.shape[1]}")
        for size in (64, 128):
            target = render.rasterize(target_commands, target_args, size=size, fill=fill, n=NPTS)
            pairs = total * size * size
            plain = lambda: ops.raster_sweep(segs, counts, size=size, fill=fill)                  # noqa: E731
            twin = lambda: ops.raster_sweep_nn(segs, counts, size=size, fill=fill)                # noqa: E731
            out, idx = twin()
            same = torch.equal(plain().view(torch.int32), out.view(torch.int32))
            live = int((idx >= 0).sum())
            (m0, lo0, hi0), (m1, lo1, hi1) = timed_ab(plain, twin, inner=10)
            print(f"[{mode} {size}] raster_sweep:     {m0 * 1e3:8.1f} us [{lo0 * 1e3:.1f} .. {hi0 * 1e3:.1f}]  {pairs / 1e9:.2f} G "
                  f"pixel-chord pairs before culling")
            print(f"[{mode} {size}] raster_sweep_nn:  {m1 * 1e3:8.1f} us [{lo1 * 1e3:.1f} .. {hi1 * 1e3:.1f}] = {m1 / m0:.2f} x "
                  f"raster_sweep; images {'bit-identical' if same else 'DIFFERENT'}; {live} live pixels = "
                  f"{live / idx.numel() * 100:.1f} % of the batch, writes {idx.numel() * 4 / 1e6:.1f} MB of indices")
            dout = (2.0 / (size * size * N) * (out - target)).contiguous()
            narrow = lambda: ops.raster_sweep_bwd(segs, counts, out, idx, dout, fill=fill, wide=False)      # noqa: E731
            wide = lambda: ops.raster_sweep_bwd(segs, counts, out, idx, dout, fill=fill, wide=True)         # noqa: E731
            (b0, blo0, bhi0), (b1, blo1, bhi1) = timed_ab(narrow, wide, inner=10)
            below = (torch.arange(segs.shape[1], device=dev).view(1, -1) < counts.view(-1, 1)).unsqueeze(-1)
            dsegs = torch.where(below, narrow(), 0)
            gap = float((dsegs - torch.where(below, wide(), 0)).abs().max())
            print(f"[{mode} {size}] raster_sweep_bwd 16 lanes per chord: {b0 * 1e3:8.1f} us [{blo0 * 1e3:.1f} .. {bhi0 * 1e3:.1f}]; a "
                  f"wave per chord: {b1 * 1e3:8.1f} us [{blo1 * 1e3:.1f} .. {bhi1 * 1e3:.1f}] = {b1 / b0:.2f} x; max |difference| "
                  f"{gap:.2e} of max |dsegs| {float(dsegs.abs().max()):.2e}")
            med_s, lo, hi = timed(lambda: ops.raster_segments_bwd(c, dsegs, counts, n=NPTS, groups=G, fill=fill), inner=20)
            print(f"[{mode} {size}] raster_segments_bwd: {med_s * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  reads "
                  f"{total * 16 / 1e6:.1f} MB of vertex gradients, writes {c.numel() * 44 / 1e6:.1f} MB")
            refined = a.clone().requires_grad_(True)
            opt = torch.optim.Adam([refined], lr=0.1)

            def step():
                opt.zero_grad(set_to_none=True)
                render.image_loss(c.view(N, G, -1), refined.view(N, G, S + 2, 11), target, fill=fill, n=NPTS)["loss"].backward()
                opt.step()
            med_r, lo, hi = timed(step, inner=5)
            print(f"[{mode} {size}] one refine_to_images step (raster_segments, raster_sweep_nn, the loss, raster_sweep_bwd, "
                  f"raster_segments_bwd, Adam): {med_r * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]")
            want = torch_loop_grad(segs, host_counts, dout, size, 3.2, fill)
            med_t, lo_t, hi_t = timed(lambda: torch_loop_grad(segs, host_counts, dout, size, 3.2, fill), inner=1, runs=3, warmup=0)
            # compared after raster_segments_bwd: where two chords tie at the vertex they share, amin's backward splits the term
            # between them and the kernel gives it to the lower index - the same vertex either way.  The largest difference is
            # that of ONE pixel within rounding of a chord (docstring of torch_loop_grad), so the median is printed next to it
            got_args = ops.raster_segments_bwd(c, dsegs, counts, n=NPTS, groups=G, fill=fill)
            want_args = ops.raster_segments_bwd(c, torch.where(below, want, 0), counts, n=NPTS, groups=G, fill=fill)
            print(f"[{mode} {size}] torch broadcast loop with autograd over {N} icons (3 runs): {med_t:8.2f} ms [{lo_t:.2f} .. "
                  f"{hi_t:.2f}] = {med_t / (m1 + b0):.0f} x raster_sweep_nn + raster_sweep_bwd; max |kernel - torch loop| in d / d args "
                  f"{float((got_args - want_args).abs().max()):.2e} (median over the non-zero elements "
                  f"{float((got_args - want_args).abs()[want_args != 0].median()):.2e}) of max {float(want_args.abs().max()):.2e}")

if __name__ == "__main__":
    main()
