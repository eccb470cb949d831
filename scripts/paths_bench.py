"""Micro-timing of the canonicalisation kernel (csrc/paths.hip) at batch 512:

  paths.canonicalize   synthetic.make_batch(512, G = 8, S = 30)            two-stage icons, 8 x 32 rows, grouped and concat
  paths.canonicalize   synthetic.make_batch_onestage(512, total_len = 50)  one-stage icons, 52 rows with several `m`
                       float32 (as the dataset and `refine` deliver them) and int64 (as greedy_sample returns them), with and
                       without numericalize = 256

HIP events around `inner` back-to-back calls, median [min .. max] of 20 such runs after warm-up, twice: launched eagerly (a
call includes the allocation of its seven outputs and the ctypes call: where the figure does not move with the shape it is
the host's enqueue cost) and as a captured graph of `inner` calls replayed (the device's time per launch, back to back).  The
bytes quoted are the input rows read once plus every output written once, over the replayed time.  No target is
stated: nobody had measured this kernel before this log.  For scale, the reference's host loop
(``SVG.from_tensors(...).canonicalize().to_tensor(...)`` through Python objects) takes about 10 ms per icon of 8 groups on one
CPU core - timed on ANOTHER machine (the build container), so the two figures are not an A/B on one box.
Writes profiles/paths_bench.log (and the same lines to stdout)."""
import os
import socket
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepsvg_amd import paths                                            # noqa: E402
from deepsvg_amd.synthetic import make_batch, make_batch_onestage         # noqa: E402

N = 512
RUNS, WARMUP, INNER = 20, 5, 20
REFERENCE_MS_PER_ICON = 10.0


def timed(fn, inner=INNER, runs=RUNS, warmup=WARMUP):
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


def graphed(fn, inner=INNER):
    """`inner` calls of fn captured once -> a function that replays them"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    return graph.replay


def main():
    assert torch.cuda.is_available(), "paths_bench.py measures on a GPU"
    dev = "cuda"
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"box {socket.gethostname()}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
    say(f"batch {N}; median [min .. max] of {RUNS} runs of {INNER} calls; reference host loop: about "
        f"{REFERENCE_MS_PER_ICON:.0f} ms per icon = {REFERENCE_MS_PER_ICON * N / 1e3:.1f} s per batch on one CPU core of another machine")
    two = make_batch(N, G=8, S=30, seed=1, device=dev)
    one = make_batch_onestage(N, total_len=50, seed=1, device=dev)
    cases = [("two-stage 8 x 32", two[0], two[1], {}),
             ("two-stage 8 x 32", two[0], two[1], {"layout": "concat", "max_seq_len": 240}),
             ("one-stage 52", one[0][:, 0], one[1][:, 0], {"max_num_groups": 8, "max_seq_len": 50, "layout": "concat"}),
             ("one-stage 52", one[0][:, 0], one[1][:, 0], {"max_num_groups": 8, "max_seq_len": 50})]
    for name, cmd, arg, kw in cases:
        for dtype in (torch.float32, torch.int64):
            for num in (None, 256):
                c, a = cmd.to(dtype).contiguous(), arg.to(dtype).contiguous()
                out = paths.canonicalize(c, a, numericalize=num, **kw)
                moved = c.numel() * c.element_size() + a.numel() * a.element_size() + sum(
                    v.numel() * v.element_size() for v in out.values())
                call = lambda: paths.canonicalize(c, a, numericalize=num, **kw)      # noqa: E731
                e_med, e_lo, e_hi = timed(call)
                med, lo, hi = (t / INNER for t in timed(graphed(call), inner=1))
                say(f"[{name} {kw.get('layout', 'grouped'):7s} {str(dtype).split('.')[-1]:7s} numericalize={num}] eager "
                    f"{e_med * 1e3:6.1f} us [{e_lo * 1e3:.1f} .. {e_hi * 1e3:.1f}], replayed {med * 1e3:6.1f} us "
                    f"[{lo * 1e3:.1f} .. {hi * 1e3:.1f}] = {med * 1e6 / N:.1f} ns per icon, {moved / 1e6:.1f} MB moved = "
                    f"{moved / med / 1e6:.0f} GB/s; valid {int(out['valid'].sum())} of {N}, {int(out['n_groups'].sum())} "
                    f"sub-paths, {int(out['reversed'].sum())} reversed; the reference's host loop is "
                    f"{REFERENCE_MS_PER_ICON * N / e_med:.0f} x an eager call (different machines)")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "paths_bench.log"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
