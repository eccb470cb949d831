"""Micro-timing of the augmenting batch assembly (dsvg_assemble_augmented, float32 store) against the plain one
(dsvg_assemble_batch, int16 store) on the same store contents, in the same process: 512 icons, G=8, S=30.  The int16 launch is
the baseline; the float store reads 48 B per row where it reads 24 B and both write the same bytes, so the expectation is a
time between 1x and (48 + w) / (24 + w) of it, w the bytes written per stored row.  Prints both times, the ratio and the
achieved bytes per second, and writes them to --log (default profiles/augment_bench.log)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepsvg_amd import dataset as D, ops, paths, svg_dataset       # noqa: E402


def timed(fn, reps=200, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "augment_bench.log"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    G, S, n_icons, N = 8, 30, 4096, 512
    icons = []
    for _ in range(n_icons):
        groups = []
        for _g in range(int(rng.integers(1, G + 1))):
            ln = int(rng.integers(2, S + 1))
            t = np.full((ln, 14), -1.0, np.float32)
            t[:, 0] = rng.integers(1, 3, size=ln)
            t[0, 0] = 0
            t[:, 8:14] = rng.integers(0, 256, size=(ln, 6))
            groups.append(t)
        icons.append([groups])
    ints = D.SVGTensorDataset(store=D.PackedSVGStore.from_icons(icons, max_num_groups=G), model_args=["commands", "args"],
                              max_num_groups=G, max_seq_len=S)
    flts = svg_dataset.SVGDataset(store=D.PackedSVGStore.from_icons(icons, max_num_groups=G, numericalized=False, viewbox=256.0),
                                  model_args=["commands", "args"], max_num_groups=G, max_seq_len=S)
    idx = torch.randint(0, n_icons, (N,), device="cuda")
    variant = ints.store.var_base[idx].to(torch.int32).contiguous()
    factor, vec = paths.augment_params(N, device="cuda")
    steps = paths._zoom_steps("bench", factor, None, 256.0) + [("translate", vec)] + paths._normalize_steps("bench", 256.0, 256)
    kinds, params = paths._pack_steps("bench", steps, N, idx.device)
    rows_read = float((ints.store.slot_off[variant.long() * G + G] - ints.store.slot_off[variant.long() * G]).sum())
    tokens = N * G * (S + 2)
    lines = [f"{torch.cuda.get_device_name(0)}; {N} icons, G={G}, S={S}: {tokens} tokens, {rows_read:.0f} stored rows per batch; "
             f"K={len(kinds)} steps (augment + numericalize); microseconds per call, mean of 200 after 10"]
    for keys in (["commands", "args"], ["commands", "args", "args_rel"]):
        rel = "args_rel" in keys
        out_b = tokens * 4 * (1 + 11 * (len(keys) - 1))
        w = out_b / rows_read
        t_int = timed(lambda: ops.assemble_batch(ints.store.rows, ints.store.slot_off, variant, G, S + 2, False, want_rel=rel))
        t_flt = timed(lambda: ops.assemble_augmented(flts.store.rows, flts.store.slot_off, variant, G, S + 2, False, kinds,
                                                     params, want_rel=rel))
        b_int = timed(lambda: ints.batch(idx, keys, random_aug=False))
        b_flt = timed(lambda: flts.batch(idx, keys))
        lines.append(f"{'+'.join(keys)}: launch int16 {t_int:.1f} us ({(out_b + 24 * rows_read) / t_int / 1e3:.1f} GB/s), float32 + "
                     f"augment {t_flt:.1f} us ({(out_b + 48 * rows_read) / t_flt / 1e3:.1f} GB/s), ratio {t_flt / t_int:.2f} "
                     f"(expected 1 .. {(48 + w) / (24 + w):.2f}, w = {w:.0f} B written per stored row)")
        lines.append(f"{'+'.join(keys)}: whole batch() call, draws and parameter packing included: SVGTensorDataset {b_int:.1f} us, "
                     f"SVGDataset {b_flt:.1f} us, ratio {b_flt / b_int:.2f}")
    # the same step program as one launch of dsvg_paths_transform over the padded batch
    padded = flts.batch(idx, ["commands", "args"], random_aug=False)
    cmd, arg = padded["commands"].contiguous(), padded["args"].contiguous()
    t_tr = timed(lambda: ops.paths_transform(cmd, arg, kinds, params, 256))
    tr_b = cmd.numel() * 4 + 2 * arg.numel() * 4
    lines.append(f"paths.transform {tuple(cmd.shape)}, K={len(kinds)}: launch {t_tr:.1f} us ({tr_b / t_tr / 1e3:.1f} GB/s of {tr_b:,} bytes "
                 f"read + written)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
