"""Micro-timing of the expansion kernel (csrc/paths_expand.hip) at 512 icons of 8 x 32 rows
(synthetic.make_batch(512, G = 8, S = 30), three `l` rows in ten turned into circular arcs for the arc op):

  paths.arcs_to_beziers   every `a` into `c` rows                        out 8 x 256 rows per icon
  paths.split             n = 2, max_dist = 2 * 256 / 24 without lines and max_dist = 7.5 * 256 / 24 with them (the first and last
                          step of the reference's simplify_heuristic)    out 8 x 256 rows per icon

HIP events around `inner` back-to-back eager calls, median [min .. max] of 20 such runs after warm-up (a call includes the
allocation of its outputs and the ctypes call).  No target is stated: nobody had measured this kernel before this log.  For
scale, the reference's host loop (``SVGPath.from_tensor(...)``, ``simplify_arcs()`` / ``split(...)``, ``to_tensor()`` through
Python objects) takes REFERENCE_MS_PER_ICON on one CPU core - timed on ANOTHER machine (the build container) on icons built the
same way, so the two figures are not an A/B on one box.
Writes profiles/paths_expand_bench.log (and the same lines to stdout)."""
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
RUNS, WARMUP, INNER = 20, 5, 20
# ms per icon of 8 groups, one CPU core of the build container: simplify_arcs, split(max_dist = 7.5 * 256 / 24)
REFERENCE_MS_PER_ICON = {"arcs_to_beziers": 20.0, "split": 22.0}


def with_arcs(commands, args, share=0.3, seed=2):
    """a share of the `l` rows as circular arcs over the same chord (radius 3/4 of the chord: lambda = 4/9)"""
    g = torch.Generator().manual_seed(seed)
    commands, args = commands.clone(), args.clone()
    pick = (commands == 1) & (torch.rand(commands.shape, generator=g).to(commands.device) < share)
    start = torch.roll(args[..., 9:11], 1, dims=2)
    radius = 0.75 * (args[..., 9:11] - start).norm(dim=-1)
    flags = torch.randint(0, 2, commands.shape + (2,), generator=g).float().to(commands.device)
    arc = torch.stack([radius, radius, torch.zeros_like(radius), flags[..., 0], flags[..., 1]], -1)
    args[..., 0:5] = torch.where(pick.unsqueeze(-1), arc, args[..., 0:5])
    commands[pick] = 3
    return commands, args


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
    assert torch.cuda.is_available(), "paths_expand_bench.py measures on a GPU"
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"box {socket.gethostname()}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
    say(f"batch {N} icons of 8 x 32 rows; median [min .. max] of {RUNS} runs of {INNER} eager calls")
    cmd, arg = make_batch(N, G=8, S=30, seed=1, device="cuda")
    acmd, aarg = with_arcs(cmd, arg)
    cases = [("arcs_to_beziers", lambda: paths.arcs_to_beziers(acmd, aarg, max_seq_len=254), acmd, aarg, "arcs_to_beziers"),
             ("split n=2", lambda: paths.split(cmd, arg, n=2, max_seq_len=254), cmd, arg, None),
             ("split max_dist=21.33 no lines", lambda: paths.split(cmd, arg, max_dist=2 * 256 / 24, include_lines=False,
                                                                   max_seq_len=254), cmd, arg, None),
             ("split max_dist=80", lambda: paths.split(cmd, arg, max_dist=7.5 * 256 / 24, max_seq_len=254), cmd, arg, "split")]
    for name, call, c, a, ref in cases:
        out = call()
        moved = c.numel() * 4 + a.numel() * 4 + sum(v.numel() * v.element_size() for v in out.values())
        med, lo, hi = timed(call)
        scale = ""
        if ref and REFERENCE_MS_PER_ICON[ref]:
            host = REFERENCE_MS_PER_ICON[ref] * N
            scale = f"; the reference's host loop: {host / 1e3:.1f} s per batch = {host / med:.0f} x (different machines)"
        say(f"[{name:30s}] eager {med * 1e3:7.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}] = {med * 1e6 / N:.0f} ns per icon, "
            f"{moved / 1e6:.1f} MB moved; valid {int(out['valid'].sum())} of {N}, rows {int((c[:, :, 1:] != 4).sum())} -> "
            f"{int(out['len_groups'].sum())}{scale}")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "paths_expand_bench.log"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
