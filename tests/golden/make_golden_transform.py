"""Generates tests/golden/paths/transform.npz by running the REAL reference (imported read-only from /root/reference) on
seeded and hand-made icons: `SVG.normalize().zoom(0.9)`, `SVGDataset._augment`, `SVGDataset.preprocess`, `SVG.rotate` and
`SVGDataset.get_data` (deepsvg/svglib/svg.py:268-300, 392-394; deepsvg/svg_dataset.py:137-215).  Run in the build container
only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_transform.py

The reference's drawing stack (cairosvg, IPython, moviepy, shapely ...) is not installed here; those modules are stubbed - the
calls above only touch numpy, torch and the reference's own geometry classes.  Icons: `m` / `l` / `c` rows in the 4 x 16 padded
layout (SOS, rows, EOS...), float coordinates in a 24 view box.  Stored for every icon what the reference returns:
  a/       normalize().zoom(0.9) of the same rows read in a 32 x 20 view box
  b/       _augment with the recorded draws (python's random.random replayed)
  c/       preprocess(augment=True, numericalize=True) with the same draws; c_mean/ preprocess(mean=True); plain/
           preprocess(augment=False): each with every key get_data produces for (G, S, T) = (4, 14, 40)
  d<k>/    rotate(Angle(deg)) for the angles in `angles`
The generator asserts that tests/paths_transform_ref.py equals the reference on every stored value (measured: equality on
numpy 2.2.6, the rotations included).
"""
import os
import random
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


class _Stub:
    def __getattr__(self, k):
        return _Stub()

    def __call__(self, *a, **k):
        return _Stub()

    def __mro_entries__(self, bases):
        return (object,)


for _name in ["cairosvg", "IPython", "IPython.display", "moviepy", "moviepy.editor", "shapely", "shapely.geometry",
              "shapely.ops", "torchvision", "torchvision.utils", "torchvision.transforms",
              "torchvision.transforms.functional", "tensorboardX", "networkx", "PIL", "PIL.Image", "PIL.ImageOps",
              "matplotlib", "matplotlib.pyplot", "matplotlib.figure", "matplotlib.colors"]:
    try:
        __import__(_name)
    except Exception:
        _m = types.ModuleType(_name)
        _m.__file__ = "/dev/null"
        _m.__getattr__ = lambda k: _Stub()
        sys.modules[_name] = _m

from deepsvg.svg_dataset import SVGDataset                     # noqa: E402
from deepsvg.svglib.geom import Angle, Bbox                    # noqa: E402
from deepsvg.svglib.svg import SVG                             # noqa: E402
from tests import paths_transform_ref as R                     # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "paths")
G, S_PAD = 4, 16
CFG = (4, 14, 40)
KEYS = ["commands", "args", "args_rel", "commands_grouped", "args_grouped", "args_rel_grouped"]
ANGLES = [90.0, 33.3, -120.0, 7.0]


def group12(cmds, pts):
    """commands and their points -> [len, 12] rows: m / l take one point (the end), c three (control1, control2, end)"""
    g = np.full((len(cmds), 12), -1.0, dtype=np.float32)
    for i, (c, p) in enumerate(zip(cmds, pts)):
        g[i, 0] = c
        p = np.asarray(p, dtype=np.float32).reshape(-1)
        g[i, 12 - len(p):] = p
    return g


def random_icon(rng):
    n_groups = int(rng.integers(1, G + 1))
    groups, left = [], CFG[2]
    for k in range(n_groups):
        ln = int(rng.integers(2, min(CFG[1], left - 2 * (n_groups - k - 1)) + 1))
        left -= ln
        cmds = [0] + [int(c) for c in rng.integers(1, 3, size=ln - 1)]
        pts = [rng.uniform(0, 24, size=6 if c == 2 else 2).astype(np.float32) for c in cmds]
        groups.append(group12(cmds, pts))
    return groups


def hand_made():
    sq = lambda a, b: group12([0, 1, 1, 1, 1], [(a, a), (b, a), (b, b), (a, b), (a, a)])
    return [
        [sq(0, 24)],                                              # the view box itself: 24 -> 256 clips to 255
        [sq(6, 18), sq(9, 15)],                                   # integers: exact under the 256 / 24 scale only by rounding
        [group12([0, 1, 2], [(0.25, 0.75), (11.953125, 12.046875), (1, 2, 3, 4, 23.75, 23.25)])],       # dyadic fractions
        [sq(12, 12.5), group12([0, 2], [(12, 12), (12, 0, 24, 12, 12, 24)])],                             # the centre
        [group12([0] + [1] * 13, [(i * 1.5, 24 - i * 1.5) for i in range(14)])],                          # a full group
        [group12([0, 1], [(0.046875, 0.0234375), (23.9765625, 23.953125)]) for _ in range(4)],            # four groups
    ]


def pad(groups):
    cmd = np.full((G, S_PAD), R.EOS, dtype=np.float32)
    args = np.full((G, S_PAD, 11), -1.0, dtype=np.float32)
    cmd[:, 0] = R.SOS
    for k, g in enumerate(groups):
        cmd[k, 1:1 + len(g)] = g[:, 0]
        args[k, 1:1 + len(g)] = g[:, 1:]
    return cmd, args


def to_svg(groups, viewbox):
    return SVG.from_tensors([torch.from_numpy(R.rows14(g)) for g in groups], viewbox=viewbox)


def back(svg):
    """the reference's tensors -> the padded args (the start positions of the 14-wide rows dropped)"""
    return pad([t.numpy()[:, [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13]] for t in svg.to_tensor(concat_groups=False)])[1]


def replay(values):
    it = iter(values)
    return lambda: float(next(it))          # python floats, as random.random returns them


def get_data(svg):
    class _Self:
        pass
    ds = _Self()
    ds.MAX_NUM_GROUPS, ds.MAX_SEQ_LEN, ds.MAX_TOTAL_LEN, ds.PAD_VAL, ds.model_args = CFG[0], CFG[1], CFG[2], -1, KEYS
    t_sep = svg.to_tensor(concat_groups=False, PAD_VAL=-1)
    res = SVGDataset.get_data(ds, t_sep, [0] * len(t_sep), model_args=KEYS)
    return {k: res[k].numpy() for k in KEYS}


if __name__ == "__main__":
    rng = np.random.default_rng(2024)
    icons = [random_icon(rng) for _ in range(24)] + hand_made()
    n = len(icons)
    u = rng.uniform(0, 1, size=(n, 3))
    draws = np.stack([5 * u[:, 0] - 2.5, 5 * u[:, 1] - 2.5, 0.2 * u[:, 2] + 0.6], axis=1)     # dx, dy, factor as python floats
    rec = {k: [] for k in ["commands", "args", "a/args", "b/args", "c/args", "c_mean/args", "plain/args"]}
    rec.update({f"d{i}/args": [] for i in range(len(ANGLES))})
    data = {tag: {k: [] for k in KEYS} for tag in ("c", "c_mean", "plain")}
    real_random = random.random
    for i, groups in enumerate(icons):
        cmd, args = pad(groups)
        rec["commands"].append(cmd)
        rec["args"].append(args)
        rec["a/args"].append(back(to_svg(groups, Bbox(32., 20.)).normalize().zoom(0.9)))
        try:
            random.random = replay(u[i])
            rec["b/args"].append(back(SVGDataset._augment(to_svg(groups, Bbox(24)))))
            random.random = replay(u[i])
            svg_c = SVGDataset.preprocess(to_svg(groups, Bbox(24)), augment=True, numericalize=True)
        finally:
            random.random = real_random
        for tag, svg in (("c", svg_c), ("c_mean", SVGDataset.preprocess(to_svg(groups, Bbox(24)), mean=True)),
                         ("plain", SVGDataset.preprocess(to_svg(groups, Bbox(24)), augment=False))):
            rec[f"{tag}/args"].append(back(svg))
            for k, v in get_data(svg).items():
                data[tag][k].append(v)
        for j, deg in enumerate(ANGLES):
            rec[f"d{j}/args"].append(back(to_svg(groups, Bbox(24)).rotate(Angle(deg))))
    rec = {k: np.stack(v) for k, v in rec.items()}
    for tag in data:
        for k in KEYS:
            rec[f"{tag}/{k}"] = np.stack(data[tag][k]).astype(np.float32)
    rec["draws"] = draws
    rec["angles"] = np.array(ANGLES)
    rec["cfg"] = np.array(CFG, dtype=np.int64)

    # the restatement equals the reference on every stored value
    cmd, args = rec["commands"], rec["args"]
    dx_dy, f = draws[:, :2], draws[:, 2]
    want = {
        "a/args": R.transform(cmd, args, R.normalize_steps((32, 20), 24) + R.zoom_steps(0.9, 24)),
        "b/args": R.transform(cmd, args, R.augment_steps(f, dx_dy, 24)),
        "c/args": R.transform(cmd, args, R.augment_steps(f, dx_dy, 24, 256), 256),
        "c_mean/args": R.transform(cmd, args, R.augment_steps(0.7, (0, 0), 24, 256), 256),
        "plain/args": R.transform(cmd, args, R.normalize_steps(24, 256), 256),
    }
    for j, deg in enumerate(ANGLES):
        want[f"d{j}/args"] = R.transform(cmd, args, R.rotate_steps(deg, 24))
    for k, w in want.items():
        diff = np.abs(w.astype(np.float64) - rec[k].astype(np.float64)).max()
        print(f"{k:12s} largest difference {diff}")
        assert np.array_equal(w, rec[k]), k
    live = (cmd < R.EOS)
    print("icons", n, "rows", int(live.sum()), "end positions and control points",
          int(live.sum() + 2 * (cmd == R.C).sum()))
    for k in list(rec):                       # the numericalised chains hold integers: stored as int16
        if k.split("/")[0] in data:
            assert np.array_equal(rec[k], np.round(rec[k])) and np.abs(rec[k]).max() < 32000
            rec[k] = rec[k].astype(np.int16)
    path = os.path.join(OUT, "transform.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")
