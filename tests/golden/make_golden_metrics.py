"""Generates tests/golden/metrics/metrics_points.npz by running the REAL reference's `SVGTensor.sample_points`
(deepsvg/difflib/tensor.py:191-230) and `chamfer_loss` (deepsvg/difflib/loss.py:5-7), imported read-only from
/root/reference, on seeded command sequences.  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py

`deepsvg.difflib.loss` pulls the reference's drawing stack in through `difflib.utils`; `chamfer_loss` is therefore taken
from the source file's own two lines by loading the module with that import stubbed.

The fixture lives in a subdirectory: tests/helpers.golden_cases() runs every tests/golden/*.npz through the model tests.

What is stored:
  commands [12, 66], args [12, 66, 11]   float32, rows past lens[i] are EOS / -1 padding (they give no points)
  lens [12]                              the reference is run on rows [:lens[i]]
  pts_n{2,7,10}, off_n{2,7,10}           the reference's points of every sequence, concatenated; sequence i owns rows
                                         off[i]:off[i + 1]
  pairs [6, 2], chamfer [6]              chamfer_loss(p.double(), q.double()) of the n = 10 clouds of six pairs - float64:
                                         the fp32 torch.cdist takes the matrix-product form on clouds of this size and is
                                         off by up to 2.8e-4 (4.8e-3 on a cloud against itself)
Sequences without a drawing command are not here: the reference raises IndexError on them.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

from deepsvg.difflib.tensor import SVGTensor                         # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics")
M, L_, C_, EOS, SOS, Z = 0, 1, 2, 4, 5, 6
L_MAX = 66
NS = (2, 7, 10)


def _chamfer_loss():
    stub = types.ModuleType("deepsvg.difflib.utils")
    stub.torch = torch
    saved = sys.modules.get("deepsvg.difflib.utils")
    sys.modules["deepsvg.difflib.utils"] = stub
    try:
        import importlib
        mod = importlib.import_module("deepsvg.difflib.loss")
    finally:
        if saved is None:
            del sys.modules["deepsvg.difflib.utils"]
        else:
            sys.modules["deepsvg.difflib.utils"] = saved
    return mod.chamfer_loss


def sequences(gen):
    def rand(k, pool):
        return [pool[i] for i in torch.randint(0, len(pool), (k,), generator=gen).tolist()]

    seqs = [
        [L_] + rand(9, [L_, C_]) + [EOS],                       # a line at row 0: starts at (0, 0)
        [SOS, L_, C_, L_, EOS],                                 # a line after SOS: starts at (-1, -1)
        [SOS, M, C_, EOS],                                      # a single drawing command
        [SOS, M] + rand(L_MAX - 2, [L_, C_]),                   # ends in a drawing command, no EOS (full length)
        [SOS, M] + rand(30, [L_, C_]) + [Z, EOS],
        [SOS, M] + rand(12, [L_, C_, Z, M]) + [C_, EOS],
        [SOS] + rand(40, [M, L_, C_, Z]) + [L_, EOS, EOS],
        rand(20, [SOS, M, L_, C_, Z, EOS]) + [C_] + rand(20, [SOS, M, L_, C_, Z, EOS]),     # commands in any order
        rand(64, [SOS, M, L_, C_, Z, EOS]) + [L_],
        [SOS, M, L_, Z, M, C_, C_, Z, EOS],
        [SOS, M] + rand(61, [C_]) + [EOS],
        [C_],                                                   # one row
    ]
    return seqs


def main():
    gen = torch.Generator().manual_seed(20240)
    chamfer_loss = _chamfer_loss()
    seqs = sequences(gen)
    n_seq = len(seqs)
    commands = torch.full((n_seq, L_MAX), EOS, dtype=torch.long)
    lens = torch.tensor([len(s) for s in seqs])
    assert int(lens.max()) <= L_MAX
    for i, s in enumerate(seqs):
        commands[i, :len(s)] = torch.tensor(s)
    vals = torch.randint(0, 256, (n_seq, L_MAX, 11), generator=gen)
    args = torch.where(SVGTensor.CMD_ARGS_MASK[commands].bool(), vals, torch.full_like(vals, -1))
    rec = {"commands": commands.numpy().astype(np.float32), "args": args.numpy().astype(np.float32),
           "lens": lens.numpy().astype(np.int32)}
    clouds = {}
    for n in NS:
        pts, off = [], [0]
        for i in range(n_seq):
            ln = int(lens[i])
            p = SVGTensor.from_cmd_args(commands[i, :ln].float(), args[i, :ln].float()).sample_points(n)
            k = int(((commands[i, :ln] == L_) | (commands[i, :ln] == C_)).sum())
            assert p.shape == (k * (n - 1) + 1, 2) and p.dtype == torch.float32
            pts.append(p)
            off.append(off[-1] + p.shape[0])
        clouds[n] = pts
        rec[f"pts_n{n}"] = torch.cat(pts).numpy()
        rec[f"off_n{n}"] = np.array(off, dtype=np.int32)
    pairs = [(0, 3), (3, 4), (5, 6), (7, 8), (10, 3), (2, 11)]
    rec["pairs"] = np.array(pairs, dtype=np.int32)
    rec["chamfer"] = np.array([chamfer_loss(clouds[10][i].double(), clouds[10][j].double()).item() for i, j in pairs],
                              dtype=np.float64)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "metrics_points.npz")
    np.savez_compressed(path, **rec)
    print(f"{path}: {os.path.getsize(path)} bytes, {n_seq} sequences, chamfer {rec['chamfer']}")


if __name__ == "__main__":
    main()
