"""Generates tests/golden/paths/simplify.npz by running the REAL reference `SVGPath.simplify` and `SVGPath.simplify_heuristic`
(deepsvg/svglib/svg_path.py:386-613, imported read-only from /root/reference) on seeded and hand-made paths.  Run in the build
container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_paths_simplify.py

The reference's drawing stack is stubbed with the stub list of make_golden_paths.py; simplify only touches numpy and torch.
Every group is an `m` followed by `l` / `c` rows (one closed by a `z`), with smooth joins in about 60 % of consecutive cubics:
one SVGPath per group.  Coordinates in the file are in the 256 box; the reference runs on them scaled by 24 / 256, and what
it returns is stored scaled back.  Stored, in the 4 x 48 layout: the icons (commands int8 [N, G, S], args float32 [N, G, S,
11], tags, family), the reference's own `split(max_dist=2, include_lines=False)` of them (pre_commands int8 [N, G, W],
pre_args float32 [N, G, W, 11]: the input of the three simplify variants), and per variant v (v_commands int8 [N, G, LO]
padded with -2, v_args float32 [N, G, LO, 11], v_len int32 [N, G]):
  fit        simplify(0.1, 0.2, 150) on the reference's own split
  default    simplify() on it
  smooth     simplify(force_smooth=True) on it
  heuristic  the whole simplify_heuristic of the icon

Screening.  The reference computes with float32 points, so near-ties decide differently.  A candidate PATH is screened with
the restatement alone (tests/paths_simplify_ref.py, its `trace` of the smallest margin of every kind of decision over all
four variants) and rejected when a threshold decision (accept, stop, break, RDP split, handle test, |det| against 1e-12)
has a relative margin below 1e-3, the worst point at which a fit or RDP splits is within 1e-3 (relative) of the runner-up
(a symmetric curve has two worst points, equal up to rounding), the normal system's |det| / (C00 C11) is below 1e-3, an alpha is within 1e-4 segLength of
its cut, two consecutive reparametrised u are closer than 1e-6, a count of the heuristic's last split is within 1e-4 of
changing, or the reference raises.  Kept paths are assembled four to an icon.  Asserted: at most half of the candidates of
each family are rejected, at least 40 icons are kept, and EVERY kept icon has the reference's structure (commands and counts
equal) in every variant.  The largest coordinate difference measured, in the reference's 24-box units, is stored as
simplify_max_abs_diff, the rejected share per family as rejected_share (short, long)."""
import math
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


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

from deepsvg.difflib.tensor import SVGTensor                    # noqa: E402
from deepsvg.svglib.svg_path import SVGPath                     # noqa: E402

import paths_expand_ref as expand_ref                           # noqa: E402
import paths_simplify_ref as ref                                # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "paths")
M, L, C, A, EOS, SOS, Z = range(7)
G, S = 4, 48
UNIT = 256 / 24
ARG_COLS = [1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13]     # the model's eleven argument columns of the 14-wide row
VARIANTS = {"fit": dict(tolerance=0.1, epsilon=0.2, angle_threshold=150.0), "default": {}, "smooth": dict(force_smooth=True)}
MARGIN = {"accept": 1e-3, "limit": 1e-3, "break": 1e-3, "rdp": 1e-3, "handle": 1e-3, "det": 1e-3, "cond": 1e-3, "argmax": 1e-3, "alpha": 1e-4,
          "order": 1e-6}
EDGE = 1e-4


def f32(v):
    return [float(x) for x in np.asarray(v, np.float32)]


def crafted():
    s_curve, p, c2 = [(M, [20, 128])], np.array([20.0, 128.0]), None
    for k in range(8):                                # eight long cubics with mirrored handles: smooth joins, > 64 points split
        e = p + np.array([27.0, 0.0])
        c1 = p + np.array([0.0, -110.0]) if c2 is None else p + (p - c2)
        c2 = e + np.array([0.0, -(100.0 + 2 * k) if k % 2 == 0 else 100.0 + 2 * k])        # not mirror images: no tied worst points
        s_curve.append((C, list(c1) + list(c2) + list(e)))
        p = e
    return [
        ([(M, [10, 20]), (L, [130, 140])], "one_line"),
        ([(M, [10, 10]), (L, [60, 12]), (L, [110, 10]), (L, [112, 90]), (L, [60, 140]), (L, [10, 90])], "polyline"),
        ([(M, [20, 200]), (C, [20, 20, 200, 40, 230, 200])], "one_long_cubic"),
        ([(M, [30, 30]), (C, [60, 10, 95, 70, 120, 30]), (L, [120, 120]), (C, [90, 150, 50, 95, 30, 120])], "c_l_c_sharp_corners"),
        ([(M, [40, 40]), (C, [80, 20, 125, 15, 160, 40]), (C, [185, 80, 175, 125, 160, 160]), (L, [40, 160]), (L, [40, 40]),
          (Z, [])], "closed_with_z"),
        (s_curve, "smooth_s_curve"),
        ([], "empty_group"),
    ]


def pack1(rows, width):
    return ref.pack([[[(c, f32(v)) for c, v in rows]]], 1, width)


def ref_path(cmd, arg):
    """the one SVGPath of a group, commands [S] / args [S, 11] in the 256 box, built in the reference's 24 box"""
    n = 0
    while 1 + n < len(cmd) and cmd[1 + n] != EOS:
        n += 1
    if not n:
        return None
    a = arg[1:1 + n].astype(np.float64)
    a = np.where(a == -1.0, -1.0, a * (24 / 256)).astype(np.float32)
    data = SVGTensor.from_cmd_args(torch.from_numpy(cmd[1:1 + n].astype(np.float32)), torch.from_numpy(a)).data
    paths = SVGPath.from_tensor(data).svg_paths
    assert len(paths) == 1
    return paths[0]


def rows_of(path):
    """-> (commands int8 [n], args float64 [n, 11] in the 256 box)"""
    if path is None:
        return np.zeros(0, np.int8), np.zeros((0, 11), np.float64)
    t = path.to_tensor().numpy().astype(np.float64)
    a = t[:, ARG_COLS]
    return t[:, 0].astype(np.int8), np.where(a == -1.0, -1.0, a * UNIT)


def run_reference(rows):
    """one path through the reference -> {"pre": rows, variant: rows}, or None when it raises"""
    cmd, arg = pack1(rows, S)
    cmd, arg = cmd[0, 0], arg[0, 0]
    out = {}
    try:
        pre = ref_path(cmd, arg)
        if pre is not None:
            pre.split(max_dist=2, include_lines=False)
        out["pre"] = rows_of(pre)
        for name, kw in VARIANTS.items():
            p = None if pre is None else pre.copy().simplify(**kw)
            out[name] = rows_of(p)
        p = ref_path(cmd, arg)
        out["heuristic"] = rows_of(None if p is None else p.simplify_heuristic())
    except ZeroDivisionError:
        return None
    return out


def as_rows(cmds, args):
    return [(int(c), f32(a[{M: 9, L: 9, C: 5, Z: 11}[int(c)]:])) for c, a in zip(cmds, args)]


def restated(rows, res):
    """the restatement on the same inputs, traced -> ({variant: dict}, trace, ok)"""
    trace, out = {}, {}
    pre = as_rows(*res["pre"])
    width = max(len(pre), len(rows)) + 2
    pc, pa = ref.pack([[pre]], 1, width)
    for name, kw in VARIANTS.items():
        out[name] = ref.simplify(pc, pa, max_seq_len=2 * width, trace=trace, **kw)
    ic, ia = pack1(rows, S)
    a = expand_ref.split(ic, ia, max_dist=2 * UNIT, include_lines=False, max_seq_len=510)
    b = ref.simplify(a["commands"], a["args"], 0.1, 0.2, 150.0, max_seq_len=510, trace=trace)
    c = expand_ref.split(b["commands"], b["args"], max_dist=7.5 * UNIT, max_seq_len=510)
    out["heuristic"] = dict(c, valid=a["valid"] & b["valid"] & c["valid"])
    lens = c["lengths"][0, 0] / (7.5 * UNIT)
    edge = any(v > 0 and abs(v - round(v)) < EDGE and round(v) >= 1 for v in lens)
    lens = a["lengths"][0, 0] / (2 * UNIT)
    edge = edge or any(v > 0 and abs(v - round(v)) < EDGE and round(v) >= 1 for v in lens)
    return out, trace, all(bool(v["valid"][0]) for v in out.values()) and not edge


def structure_equal(ours, theirs):
    n = int(ours["len_groups"][0, 0])
    return n == len(theirs[0]) and np.array_equal(ours["commands"][0, 0, 1:1 + n], theirs[0].astype(np.float32))


def coordinate_diff(ours, theirs):
    """largest difference over the enabled slots, in the reference's units"""
    n = len(theirs[0])
    if not n:
        return 0.0
    live = ref.enabled(theirs[0])
    d = np.abs(ours["args"][0, 0, 1:1 + n].astype(np.float64) - theirs[1]) / UNIT
    return float(d[live].max(initial=0.0))


def screen(rows):
    """-> (reference results, restated results, reason it is rejected or None)"""
    res = run_reference(rows)
    if res is None:
        return None, None, "raises"
    out, trace, ok = restated(rows, res)
    if not ok:
        return res, out, "invalid or near a split count"
    for kind, least in MARGIN.items():
        if trace.get(kind, math.inf) < least:
            return res, out, kind
    return res, out, None


if __name__ == "__main__":
    rng = np.random.default_rng(2026)
    kept, stats, worst, unscreened_differ = [], {}, 0.0, 0
    for rows, tag in crafted():
        res, out, why = screen(rows)
        assert why is None, (tag, why)
        kept.append((rows, tag, "crafted", res, out))
    for family, lo, hi, want in (("short", 1, 5, 112), ("long", 4, 11, 44)):
        tried = rejected = got = 0
        while got < want:
            rows = ref.smooth_path(rng, int(rng.integers(lo, hi + 1)))
            rows = [(c, f32(v)) for c, v in rows]
            tried += 1
            res, out, why = screen(rows)
            if why is not None:
                rejected += 1
                if res is not None and not all(structure_equal(out[k], res[k]) for k in out):
                    unscreened_differ += 1
                continue
            kept.append((rows, "random", family, res, out))
            got += 1
        stats[family] = rejected / tried
        print(family, "tried", tried, "rejected", rejected, f"({100 * rejected / tried:.0f} %)")
        assert rejected <= tried / 2, family
    print("rejected candidates whose structure differs from the reference's:", unscreened_differ)

    # EVERY kept path has the reference's structure, in every variant
    for rows, tag, family, res, out in kept:
        for name in out:
            assert structure_equal(out[name], res[name]), (tag, family, name)
            worst = max(worst, coordinate_diff(out[name], res[name]))
            if coordinate_diff(out[name], res[name]) > 1e-3:
                print("  large difference:", tag, family, name, coordinate_diff(out[name], res[name]))
    print("kept", len(kept), "paths; largest coordinate difference", worst, "reference units")

    n_icons = (len(kept) + G - 1) // G
    assert n_icons >= 40, n_icons
    icons = [kept[i * G:(i + 1) * G] for i in range(n_icons)]
    cmd, arg = ref.pack([[k[0] for k in icon] for icon in icons], G, S)
    rec = dict(commands=cmd.astype(np.int8), args=arg,
               tags=np.array([[k[1] for k in icon] + [""] * (G - len(icon)) for icon in icons]),
               family=np.array([[k[2] for k in icon] + [""] * (G - len(icon)) for icon in icons]),
               simplify_max_abs_diff=np.float64(worst), rejected_share=np.array([stats["short"], stats["long"]]))
    for name in ["pre"] + list(VARIANTS) + ["heuristic"]:
        lo = max(len(k[3][name][0]) for k in kept)
        oc = np.full((n_icons, G, lo), -2, np.int8)
        oa = np.full((n_icons, G, lo, 11), -1.0, np.float32)
        ln = np.zeros((n_icons, G), np.int32)
        for b, icon in enumerate(icons):
            for g, k in enumerate(icon):
                c, a = k[3][name]
                ln[b, g] = len(c)
                oc[b, g, :len(c)] = c
                oa[b, g, :len(c)] = a.astype(np.float32)
        rec[f"{name}_commands"], rec[f"{name}_args"], rec[f"{name}_len"] = oc, oa, ln
        print(name, "LO", lo, "rows", int(ln.sum()))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "simplify.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024
