"""Micro-timing of the Bezier fit (csrc/paths_simplify.hip) at 512 icons of 8 x 32 rows (synthetic.make_batch(512, G = 8, S = 30)):

  paths.simplify             tolerance 0.1, epsilon 0.2, angle_threshold 150 on the batch as split(max_dist = 2 * 256 / 24,
                             include_lines=False) leaves it (8 x 256 rows per icon in and out): the middle step of the
                             reference's simplify_heuristic on its own
  paths.simplify_heuristic   the three launches, 8 x 256 work rows and 8 x 256 rows out per icon

HIP events around `inner` back-to-back eager calls, median [min .. max] of 20 such runs after warm-up (a call includes the
allocation of its outputs and workspace and the ctypes calls).  No target is stated: nobody had measured this kernel before this
log.  For scale, the reference's host loop (``SVGPath.from_tensor(...)``, ``simplify(...)`` / ``simplify_heuristic()``,
``to_tensor()`` through Python objects) takes REFERENCE_MS_PER_ICON on one CPU core - timed on ANOTHER machine (the build
container, with the path construction of tests/golden/make_golden_paths_simplify.py) on icons built the same way, so the two
figures are not an A/B on one box.
Writes profiles/paths_simplify_bench.log (and the same lines to stdout)."""
import os
import socket
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepsvg_amd import paths                                            # noqa: E402
from deepsvg_amd.synthetic import make_batch                             # noqa: E402

N = 512
RUNS, WARMUP, INNER = 20, 5, 10
UNIT = 256 / 24
# ms per icon of 8 groups, one CPU core of the build container: simplify(0.1, 0.2, 150) of the split icon, simplify_heuristic()
REFERENCE_MS_PER_ICON = {"simplify": 69.0, "simplify_heuristic": 94.0}


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


def main():
    assert torch.cuda.is_available(), "paths_simplify_bench.py measures on a GPU"
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"box {socket.gethostname()}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
    say(f"batch {N} icons of 8 x 32 rows; median [min .. max] of {RUNS} runs of {INNER} eager calls")
    cmd, arg = make_batch(N, G=8, S=30, seed=1, device="cuda")
    pre = paths.split(cmd, arg, max_dist=2 * UNIT, include_lines=False, max_seq_len=254)
    pcmd, parg = pre["commands"], pre["args"]
    cases = [("simplify", lambda: paths.simplify(pcmd, parg, 0.1, 0.2, 150.0, max_seq_len=254), pcmd),
             ("simplify_heuristic", lambda: paths.simplify_heuristic(cmd, arg, max_seq_len=254), cmd)]
    for name, call, c in cases:
        out = call()
        med, lo, hi = timed(call)
        host = REFERENCE_MS_PER_ICON[name] * N
        say(f"[{name:20s}] eager {med * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}] = {med * 1e3 / N:.2f} us per icon; valid "
            f"{int(out['valid'].sum())} of {N}, rows {int((c[:, :, 1:] != 4).sum())} -> {int(out['len_groups'].sum())}; the "
            f"reference's host loop: {host / 1e3:.1f} s per batch = {host / med:.0f} x (different machines)")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "paths_simplify_bench.log"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
