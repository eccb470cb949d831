"""Generates tests/golden/paths/canonicalize.npz by running the REAL reference canonicalisation,
`deepsvg.svglib.svg.SVG.from_tensors(...).canonicalize()` (imported read-only from /root/reference), on seeded and hand-made
icons, and `_apply_to_paths("numericalize", 256)` on its result for the rounded variant.  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_paths.py

The reference's drawing stack (cairosvg, IPython, moviepy, shapely ...) is not installed here; those modules are stubbed with
the stub list of make_golden_batch.py - canonicalize itself only touches numpy and torch.  Stored, as padded arrays: the input
icons (commands int8 [N, G, S] with SOS / EOS framing, args float32 [N, G, S, 11]), what the reference returns for each
(out_commands int8 [N, GO, LO] padded with -2, out_args float32 [N, GO, LO, 11], the same after numericalize(256), out_n int32
[N] groups, out_len int32 [N, GO] rows per group), a tag per icon naming the case it covers, and the pairs of squared norms on
the 256 x 256 integer grid where the float32 and the float64 form of the rotation's norm test disagree."""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")


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
from deepsvg.svglib.geom import Bbox                            # noqa: E402
from deepsvg.svglib.svg import SVG                              # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "paths")
M, L, C, A, EOS, SOS, Z = range(7)
G, S = 4, 16                                    # input layout: 4 groups of SOS + up to 14 rows + EOS
ARG_COLS = [1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13]     # the model's eleven argument columns of the 14-wide row


def pack(groups):
    """groups: <= G lists of (command, values): m / l -> [x, y], c -> [c1x, c1y, c2x, c2y, x, y], z -> []"""
    cmd = np.full((G, S), EOS, np.int8)
    arg = np.full((G, S, 11), -1.0, np.float32)
    cmd[:, 0] = SOS
    assert len(groups) <= G
    for g, seq in enumerate(groups):
        assert len(seq) <= S - 2
        for r, (c, v) in enumerate(seq, 1):
            cmd[g, r] = c
            if c in (M, L):
                arg[g, r, 9:11] = v
            elif c == C:
                arg[g, r, 5:11] = v
    return cmd, arg


def reference(cmd, arg):
    """the rows between SOS and the first EOS of every non-empty group -> SVG.from_tensors -> canonicalize -> to_tensor,
    before and after numericalize(256)"""
    tensors = []
    for g in range(G):
        rows = [r for r in range(1, S) if cmd[g, r] != EOS]
        n = 0
        while n < S - 1 and cmd[g, 1 + n] != EOS:
            n += 1
        assert rows == list(range(1, 1 + n))
        if n:
            tensors.append(SVGTensor.from_cmd_args(torch.from_numpy(cmd[g, 1:1 + n].astype(np.float32)),
                                                   torch.from_numpy(arg[g, 1:1 + n].copy())).data)
    svg = SVG.from_tensors(tensors, viewbox=Bbox(256))
    svg.canonicalize()
    raw = [t.numpy().copy() for t in svg.to_tensor(concat_groups=False)]
    svg._apply_to_paths("numericalize", 256)
    rounded = [t.numpy().copy() for t in svg.to_tensor(concat_groups=False)]
    return raw, rounded


def norm_pairs():
    """ordered pairs (a, b) of squared norms x^2 + y^2, 0 <= x, y <= 255, where np.isclose(norm a, norm b) differs between
    the float32 norms the reference takes (Point.norm of a float32 pair) and float64 norms"""
    sq = sorted({x * x + y * y for x in range(256) for y in range(256)})
    have = set(sq)
    pairs = []
    for a in sq:
        for b in (a - 2, a - 1, a + 1, a + 2):      # |sqrt a - sqrt b| <= 1e-5 sqrt b needs |a - b| <= 2e-5 b < 3
            if b in have and b > 0:
                na32, nb32 = np.sqrt(np.float32(a)), np.sqrt(np.float32(b))
                c32 = abs(float(np.float32(na32 - nb32))) <= 1e-8 + 1e-5 * abs(float(nb32))
                c64 = abs(np.sqrt(float(a)) - np.sqrt(float(b))) <= 1e-8 + 1e-5 * np.sqrt(float(b))
                if c32 != c64:
                    pairs.append((a, b))
    return pairs


def points_of(sqn):
    return [(x, y) for x in range(256) for y in range(256) if x * x + y * y == sqn]


def norm_icons(pairs):
    """closed sub-paths m q, l p, l r, l q, z whose rotation the norm test decides: p below q (p.y > q.y) and left of it
    (p.x < q.x), |p|^2 = a, |q|^2 = b, r far down-right so that it never wins"""
    icons = []
    for a, b in pairs:
        found = None
        for p in points_of(a):
            for q in points_of(b):
                if p[1] > q[1] and p[0] < q[0] and max(p[1], q[1]) < 250:
                    found = (p, q)
                    break
            if found:
                break
        if found:
            p, q = found
            r = (255, 255)
            icons.append(([[(M, list(q)), (L, list(p)), (L, list(r)), (L, list(q)), (Z, [])]], f"norm32_{a}_{b}"))
    return icons


def crafted():
    sq = [(M, [50, 50]), (L, [50, 90]), (L, [90, 90]), (L, [90, 50]), (L, [50, 50])]
    return [
        ([[(M, [10, 20]), (L, [30, 40])]], "m_l_only"),
        ([], "empty_icon"),
        ([[], [], []], "empty_groups"),
        ([[(L, [5, 5]), (C, [1, 2, 3, 4, 9, 9]), (M, [20, 20]), (L, [40, 20]), (L, [40, 60]), (Z, []), (L, [1, 1]),
           (C, [1, 1, 2, 2, 3, 3]), (M, [3, 200]), (L, [3, 100])]], "rows_before_m_and_after_z"),
        ([[(M, [100, 100]), (L, [120, 100]), (L, [120, 130]), (M, [10, 10]), (L, [5, 40]), (L, [30, 40]), (Z, []),
           (M, [60, 5]), (C, [70, 0, 80, 0, 90, 5]), (L, [90, 30])]], "three_subpaths_in_a_group"),
        ([[(M, [10, 10]), (L, [10, 10]), (C, [20, 20, 30, 30, 10, 10]), (M, [40, 40]), (L, [50, 60])]],
         "subpath_of_degenerate_commands_only"),
        ([[(M, [30, 30]), (L, [60, 30]), (C, [90, 0, 90, 90, 60, 30]), (L, [60, 80]), (L, [30, 30])]],
         "degenerate_bezier_loop"),
        ([[(M, [40, 10]), (L, [40, 90])], [(M, [70, 90]), (L, [70, 10])], [(M, [10, 50]), (L, [90, 50])],
          [(M, [90, 60]), (L, [10, 60])]], "one_command_subpaths_both_orientations"),
        ([[(M, [20, 20]), (L, [60, 20]), (L, [60, 60])], [(M, [20, 20]), (L, [20, 60]), (L, [60, 60])],
          [(M, [20, 20]), (C, [30, 10, 50, 10, 70, 70]), (L, [10, 70])], [(M, [5, 20]), (L, [9, 9]), (L, [1, 1])]],
         "equal_start_keys_stable_order"),
        ([[(M, [10, 10]), (L, [20, 20]), (L, [40, 40])], [(M, [0, 0]), (L, [50, 0]), (L, [0, 0])]], "determinant_sum_zero"),
        ([[(M, [10, 10]), (L, [10, 200]), (L, [200, 200])], [(M, [100, 20]), (L, [150, 20]), (L, [150, 60])]],
         "reversed_start_breaks_sort_order"),
        ([[*sq[:1], *sq[1:], (Z, [])], [(M, [90, 190]), (L, [20, 110]), (L, [150, 120]), (L, [90, 190]), (Z, [])]],
         "closed_without_gap_rotated"),
        ([[(M, [50, 50]), (L, [90, 50]), (L, [20, 10]), (Z, [])], [(M, [200, 200]), (L, [150, 220]), (L, [120, 130]),
                                                                   (L, [180, 140]), (Z, [])]], "closed_with_gap_rotated"),
        ([[(M, [100, 100]), (C, [110, 80, 130, 80, 140, 100]), (C, [150, 130, 120, 150, 100, 140]), (L, [60, 120]),
           (C, [50, 110, 70, 100, 100, 100]), (Z, [])], [(M, [10, 10]), (C, [12, 40, 30, 60, 5, 80])]], "c_commands_reversed"),
        ([[(M, [10.25, 20.5]), (L, [30.5, 40.5]), (C, [1.5, 2.5, 3.5, 4.5, 0.5, 255.5]), (L, [254.5, 255.75])],
          [(M, [100.5, 7.25]), (L, [60.75, 90.5]), (L, [140.25, 80.5]), (L, [100.5, 7.25]), (Z, [])],
          [(M, [5.5, 5.5]), (L, [5.5, 5.50001]), (L, [6.5, 5.5])]], "float_coordinates"),
        ([[(M, [0.5, 1.5]), (L, [2.5, 3.5]), (L, [-3.5, 300.25]), (C, [-0.5, 254.5, 255.5, 256.5, 17.5, 18.5])]],
         "float_half_values_and_clipping"),
        ([[(M, [10, 10]), (M, [20, 20]), (L, [30, 30]), (Z, []), (Z, []), (M, [1, 1]), (Z, []), (L, [2, 2])]],
         "consecutive_markers"),
        ([[(M, [10, 10]), (L, [40, 10]), (L, [40, 40]), (L, [10, 40]), (L, [10, 10])],
          [(M, [60, 60]), (L, [90, 60]), (L, [90, 90]), (L, [60, 90]), (L, [60, 60])],
          [(M, [60, 100]), (C, [70, 90, 90, 90, 100, 100]), (C, [90, 120, 70, 120, 60, 100])]], "already_canonical"),
    ]


def random_icon(rng, small):
    hi = 8 if small else 256
    groups = []
    for _ in range(int(rng.integers(1, G + 1))):
        seq = []
        for i in range(int(rng.integers(0, S - 1))):
            c = int(rng.choice([M, L, L, C, C, Z, L, L, C, L, C, L])) if i else int(rng.choice([M, M, M, L, C]))
            n = {M: 2, L: 2, C: 6, Z: 0}[c]
            seq.append((c, [float(v) for v in rng.integers(0, hi, size=n)]))
        groups.append(seq)
    return groups


if __name__ == "__main__":
    pairs = norm_pairs()
    icons = crafted() + norm_icons(pairs)
    n_norm = len(icons) - len(crafted())
    rng = np.random.default_rng(2024)
    icons += [(random_icon(rng, small=False), "random") for _ in range(150)]
    icons += [(random_icon(rng, small=True), "random_small_grid") for _ in range(100)]      # duplicates, ties, zero sums

    cmds, args, raws, rounds, tags = [], [], [], [], []
    for groups, tag in icons:
        c, a = pack(groups)
        raw, rounded = reference(c, a)
        cmds.append(c), args.append(a), raws.append(raw), rounds.append(rounded), tags.append(tag)
    GO = max(len(r) for r in raws)
    LO = max([len(t) for r in raws for t in r])
    N = len(icons)
    rec = {"commands": np.stack(cmds), "args": np.stack(args), "tags": np.array(tags),
           "norm_pairs": np.array(pairs, dtype=np.int32),
           "out_commands": np.full((N, GO, LO), -2, np.int8), "out_n": np.zeros(N, np.int32),
           "out_len": np.zeros((N, GO), np.int32)}
    for key, res in (("out_args", raws), ("out_args_256", rounds)):
        rec[key] = np.full((N, GO, LO, 11), -1.0, np.float32)
        for b, groups in enumerate(res):
            rec["out_n"][b] = len(groups)
            for k, t in enumerate(groups):
                rec["out_len"][b, k] = len(t)
                rec["out_commands"][b, k, :len(t)] = t[:, 0].astype(np.int8)
                rec[key][b, k, :len(t)] = t[:, ARG_COLS]
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "canonicalize.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes;", N, "icons,", len(pairs), "norm pairs,", n_norm,
          "of them in closed sub-paths; GO", GO, "LO", LO)
