"""Micro-timing of the rasteriser kernels (csrc/raster.hip) at batch 512, hierarchical_ordered shapes (G = 8 groups of
S + 2 = 32 tokens) of deepsvg_amd.synthetic's typical fill (1..8 visible groups, 2..30 commands each), n = 10:

  ops.raster_segments  stroke and fill, float32 targets (as the dataset delivers them)
  ops.raster_sweep     sizes 64 and 128, stroke and fill, cull = 0 and cull = 1: the two arms ALTERNATE inside one process, and
                       their images are compared in bits
  the same definition as plain torch on the same GPU: a loop over icons of one [pixels, chords] fp32 broadcast each, from
                       the kernel's own chord records (counts on the host) - what one would write without the kernels

HIP events around `inner` back-to-back calls, median [min .. max] of 20 such runs after warm-up.  The pixel-chord pairs are
counted from the chord counts; the quoted VALU floor is pairs * OPS vector instructions (stroke 12: two subtractions, the
dot product, the clamped parameter, the closest point, the squared length, the minimum; fill 24 with the crossing test) over
256 CUs * 4 SIMDs * 32 lanes per clock at 2.4 GHz.  Writes nothing but stdout."""
import os
import socket
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsvg_amd import ops                          # noqa: E402
from deepsvg_amd.synthetic import make_batch         # noqa: E402

N, G, S, NPTS = 512, 8, 30, 10
RUNS, WARMUP = 20, 5
VALU_LANES_PER_S = 256 * 4 * 32 * 2.4e9
OPS = {False: 12, True: 24}


def timed(fn, inner, runs=RUNS, warmup=WARMUP):
    """-> (median, min, max) ms per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def timed_ab(fa, fb, inner, runs=RUNS, warmup=WARMUP):
    """the two arms alternating, run by run -> ((median, min, max) of a, of b) ms per call"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(runs):
        for arm, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[arm].append(e0.elapsed_time(e1) / inner)
    return tuple((statistics.median(m), min(m), max(m)) for m in ms)


def torch_loop(segs, counts, size, stroke_width, fill):
    """the definition of include/dsvg.h one icon at a time: [chords, size, size] fp32 broadcasts (counts on the host)"""
    s = 256.0 / size
    centre = (torch.arange(size, device=segs.device, dtype=torch.float32) + 0.5) * s
    cx, cy = centre.view(1, 1, size), centre.view(1, size, 1)
    out = torch.zeros(segs.shape[0], size, size, device=segs.device)
    for i, k in enumerate(counts):
        if k == 0:
            continue
        r = segs[i, :k]
        ax, ay, dx, dy = (r[:, j].view(-1, 1, 1) for j in range(4))
        px, py = cx - ax, cy - ay
        len2 = dx * dx + dy * dy
        t = ((px * dx + py * dy) / len2.clamp(min=1e-30)).clamp(0, 1)
        d = ((px - t * dx) ** 2 + (py - t * dy) ** 2).amin(0).sqrt()
        if not fill:
            out[i] = (0.5 + (stroke_width / 2 - d) / s).clamp(0, 1)
            continue
        by = ay + dy
        right = (ax + py * dx / torch.where(dy != 0, dy, torch.ones_like(dy))) > cx
        w = (((ay <= cy) & (cy < by) & right).to(torch.int32) - ((by <= cy) & (cy < ay) & right).to(torch.int32))
        seq = (r[:, 4].contiguous().view(torch.int32) & 1).long().cumsum(0) - 1
        wind = torch.zeros(int(seq[-1]) + 1, size, size, dtype=torch.int32, device=segs.device).index_add_(0, seq, w)
        out[i] = torch.where((wind != 0).any(0), 0.5 + d / s, 0.5 - d / s).clamp(0, 1)
    return out


def main():
    assert torch.cuda.is_available(), "raster_bench.py measures on a GPU"
    dev = "cuda"
    print(f"box {socket.gethostname()}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
    print(f"batch {N}, G = {G}, S + 2 = {S + 2}, n = {NPTS}, typical fill; median [min .. max] of {RUNS} runs")
    commands, args = make_batch(N, G=G, S=S, seed=1, device=dev)
    c, a = commands.reshape(N * G, S + 2).contiguous(), args.reshape(N * G, S + 2, 11).contiguous()
    for fill in (False, True):
        mode = "fill" if fill else "stroke"
        med, lo, hi = timed(lambda: ops.raster_segments(c, a, n=NPTS, groups=G, fill=fill), inner=20)
        segs, counts = ops.raster_segments(c, a, n=NPTS, groups=G, fill=fill)
        total = int(counts.sum())
        print(f"[{mode}] raster_segments: {med * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  {total} chords, mean "
              f"{total / N:.0f} / max {int(counts.max())} per image, {total * 20 / 1e6:.1f} MB of records in a "
              f"{segs.numel() * 4 / 1e6:.1f} MB buffer")
        host_counts = counts.tolist()
        for size in (64, 128):
            pairs = total * size * size
            floor_ms = pairs * OPS[fill] / VALU_LANES_PER_S * 1e3
            plain = lambda: ops.raster_sweep(segs, counts, size=size, fill=fill, cull=False)      # noqa: E731
            culled = lambda: ops.raster_sweep(segs, counts, size=size, fill=fill, cull=True)      # noqa: E731
            same = torch.equal(plain().view(torch.int32), culled().view(torch.int32))
            (m0, lo0, hi0), (m1, lo1, hi1) = timed_ab(plain, culled, inner=10)
            print(f"[{mode} {size}] raster_sweep cull=0: {m0 * 1e3:8.1f} us [{lo0 * 1e3:.1f} .. {hi0 * 1e3:.1f}]  "
                  f"{pairs / 1e9:.2f} G pixel-chord pairs, {pairs / m0 / 1e9:.1f} T pairs/s; VALU floor {floor_ms * 1e3:.1f} us = "
                  f"{floor_ms / m0 * 100:.0f} % of the launch")
            print(f"[{mode} {size}] raster_sweep cull=1: {m1 * 1e3:8.1f} us [{lo1 * 1e3:.1f} .. {hi1 * 1e3:.1f}] = "
                  f"{m1 / m0:.2f} x cull=0; images {'bit-identical' if same else 'DIFFERENT'}")
            got = plain()
            want = torch_loop(segs, host_counts, size, 3.2, fill)
            med_t, lo_t, hi_t = timed(lambda: torch_loop(segs, host_counts, size, 3.2, fill), inner=1, runs=5, warmup=1)
            print(f"[{mode} {size}] torch broadcast loop over {N} icons (5 runs): {med_t:8.2f} ms [{lo_t:.2f} .. {hi_t:.2f}] = "
                  f"{med_t / (med + m0):.0f} x segments + sweep; largest broadcast "
                  f"{max(host_counts) * size * size * 4 / 1e6:.1f} MB per temporary; max |kernel - torch loop| "
                  f"{float((got - want).abs().max()):.2e}, mean ink {float(got.mean()):.4f}")


if __name__ == "__main__":
    main()
