"""Generates tests/golden/paths/expand.npz by running the REAL reference `SVGPath.split` and `SVGPath.simplify_arcs`
(deepsvg/svglib/svg_path.py:615-630, 280-293, imported read-only from /root/reference) on seeded and hand-made icons.  Run in
the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_paths_expand.py

The reference's drawing stack is stubbed with the stub list of make_golden_paths.py; split and simplify_arcs only touch numpy and
torch.  Every group is `m`, then `l` / `c` (split icons) or `l` / `c` / `a` (arc icons) rows, some closed by a `z`: one SVGPath
per group, whose path_commands are the rows behind the `m`.  Stored, as padded arrays in the 4 x 16 layout of
canonicalize.npz: the split icons (split_commands int8 [N, G, S], split_args float32 [N, G, S, 11]) and what the reference
returns for n in {1, 2, 5} and max_dist in {2 * 256 / 24, 7.5 * 256 / 24} with include_lines both ways (per variant v:
v_commands int8 [N, G, LO] padded with -2, v_args float32 [N, G, LO, 11], v_len int32 [N, G]; split_lengths float64 [N, G, S]:
the reference's own `length()` of every `l` / `c`); the arc icons and `simplify_arcs` of them in the same form (arcs_*), with a
tag per icon.

A case is rejected when a count could depend on the last bit: length / max_dist, or |sweep| / 45, within 1e-6 of an integer (in
the float64 restatement, tests/paths_expand_ref.py).  The one exception are the hand-made axis-aligned arcs the set has to
hold (semicircles, a quarter and a three-quarter arc): there the sweep IS a multiple of 45 degrees, and it is so exactly, in
the reference and in the restatement alike, because every intermediate value is a small integer and acos(-1) and acos(0) are
the constants pi and pi / 2 - the generator asserts that both sweeps are exactly equal to the multiple.  Arcs with radii too
small for their chord and those close to it (lambda > 0.98; the hand-made semicircles have lambda = 1 exactly, which is not
above 1 in either arithmetic) and arcs with exactly one radius 0 are left out: the op deviates from the reference there on
purpose.  The largest absolute difference between the restatement's and the reference's coordinates is stored per op
(split_max_abs_diff, arcs_max_abs_diff), and the largest difference of the lengths relative to max(length, 1)
(length_max_rel_diff for `c`, line_length_max_rel_diff for `l`, whose norm the reference takes in float32)."""
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
from deepsvg.svglib.svg_command import SVGCommandArc, SVGCommandBezier, SVGCommandLine        # noqa: E402
from deepsvg.svglib.svg_path import SVGPath                     # noqa: E402

import paths_expand_ref as ref                                  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "paths")
M, L, C, A, EOS, SOS, Z = range(7)
G, S = 4, 16
ARG_COLS = [1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13]     # the model's eleven argument columns of the 14-wide row
MAX_DISTS = {"d2": 2 * 256 / 24, "d7": 7.5 * 256 / 24}
NS = (1, 2, 5)
EDGE = 1e-6


def pack(groups):
    """groups: <= G lists of (command, values): m / l -> [x, y], c -> [c1x, c1y, c2x, c2y, x, y], a -> [rx, ry, phi, fA, fS,
    x, y], z -> []"""
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
            elif c == A:
                arg[g, r, 0:5] = v[:5]
                arg[g, r, 9:11] = v[5:]
    return cmd, arg


def ref_paths(cmd, arg, g):
    n = 0
    while n < S - 1 and cmd[g, 1 + n] != EOS:
        n += 1
    if not n:
        return []
    data = SVGTensor.from_cmd_args(torch.from_numpy(cmd[g, 1:1 + n].astype(np.float32)),
                                   torch.from_numpy(arg[g, 1:1 + n].copy())).data
    paths = SVGPath.from_tensor(data).svg_paths
    assert len(paths) == 1 and len(paths[0].path_commands) == n - 1 - int(cmd[g, n] == Z)
    return paths


def run_reference(cmd, arg, op):
    """op(path) on the one path of every group -> per group the [rows, 11] float32 array the reference returns ([] if empty)"""
    out = []
    for g in range(G):
        paths = ref_paths(cmd, arg, g)
        for p in paths:
            op(p)
        if paths:
            t = torch.cat([p.to_tensor() for p in paths]).numpy()
            out.append((t[:, 0].astype(np.int8), t[:, ARG_COLS].astype(np.float32)))
        else:
            out.append((np.zeros(0, np.int8), np.zeros((0, 11), np.float32)))
    return out


def near_integer(q, first):
    """q within EDGE of an integer at which the count changes: `first` is the lowest such integer (max(ceil(q), 1) changes at
    1, 2, ...; max(floor(q), 1) at 2, 3, ...)"""
    return round(q) >= first and abs(q - round(q)) < EDGE


def ref_lengths(cmd, arg):
    """the reference's own length() of every l / c row, float64 [G, S]"""
    out = np.zeros((G, S), np.float64)
    for g in range(G):
        for p in ref_paths(cmd, arg, g):
            for r, c in enumerate(p.path_commands, 2):
                if isinstance(c, (SVGCommandLine, SVGCommandBezier)):
                    out[g, r] = float(c.length())
    return out


def split_ok(cmd, arg):
    """no count of this icon depends on the last bit, for either max_dist"""
    lens = lengths64(cmd, arg)
    return not any(near_integer(v / d, 1) for v in lens.ravel() if v > 0 for d in MAX_DISTS.values())


def lengths64(cmd, arg):
    """the restatement's float64 lengths of one icon, [G, S]"""
    _, lens, ok = ref.expand_icon(cmd.astype(np.float32), arg, 2048, False, 1, 0.0, True)
    assert ok
    return lens


def arc_facts(cmd, arg):
    """per live `a` row: (group, row, the restatement's parameters)"""
    out = []
    for g in range(G):
        for r in range(1, S):
            if cmd[g, r] == EOS:
                break
            if cmd[g, r] == A:
                a = arg[g, r]
                par = ref.arc_parameters(float(arg[g, r - 1, 9]), float(arg[g, r - 1, 10]), *[float(v) for v in a[0:5]],
                                         float(a[9]), float(a[10]))
                out.append((g, r, par))
    return out


def arcs_ok(cmd, arg, exact):
    """lambda <= 0.98, no single zero radius, no sweep within EDGE of a multiple of 45 degrees - or, for the hand-made icons
    (exact), the sweep exactly such a multiple in the restatement and in the reference"""
    for g, r, par in arc_facts(cmd, arg):
        assert par is not None
        if par == ref.DROP:
            continue
        if par == ref.LINE or par["lam"] > (1.0 if exact else 0.98):      # a hand-made semicircle has lambda = 1 exactly
            return False
        q = abs(par["dth"]) / 45.0
        if near_integer(q, 2):
            if not exact:
                return False
            rc = ref_paths(cmd, arg, g)[0].path_commands[r - 2]
            assert isinstance(rc, SVGCommandArc)
            _, _, dth = rc._get_center_parametrization()
            assert q == round(q) and float(dth.deg) == par["dth"], (q, dth.deg, par["dth"])
    return True


def random_split_icon(rng):
    groups = []
    for _ in range(int(rng.integers(1, G + 1))):
        seq = [(M, [float(v) for v in rng.uniform(0, 256, 2).astype(np.float32)])]
        for _ in range(int(rng.integers(1, 5))):
            c = int(rng.choice([L, C, C]))
            span = float(rng.choice([8.0, 40.0, 256.0]))
            last = np.array(seq[-1][1][-2:])
            pts = np.clip(last + rng.uniform(-span, span, (3, 2)), 0, 255.9).astype(np.float32)
            seq.append((c, [float(v) for v in (pts[2] if c == L else pts.ravel())]))
        if rng.random() < 0.3:
            seq.append((Z, []))
        groups.append(seq)
    return groups


def arc_between(rng, s):
    """an arc from s with radii large enough for its chord"""
    e = np.clip(s + rng.uniform(-120, 120, 2), 0, 255.9).astype(np.float32)
    half = 0.5 * float(np.hypot(*(e - s)))
    r = (half * rng.uniform(1.05, 3.0, 2)).astype(np.float32) + np.float32(0.5)
    phi = np.float32(rng.uniform(-180, 180))
    return (A, [float(r[0]), float(r[1]), float(phi), float(rng.integers(0, 2)), float(rng.integers(0, 2)), float(e[0]),
                float(e[1])])


def random_arc_icon(rng):
    groups = []
    for _ in range(int(rng.integers(1, G + 1))):
        seq = [(M, [float(v) for v in rng.uniform(20, 236, 2).astype(np.float32)])]
        for _ in range(int(rng.integers(1, 5))):
            c = int(rng.choice([L, C, A, A, A]))
            last = np.array(seq[-1][1][-2:], np.float32)
            if c == A:
                seq.append(arc_between(rng, last))
            else:
                pts = np.clip(last + rng.uniform(-60, 60, (3, 2)), 0, 255.9).astype(np.float32)
                seq.append((c, [float(v) for v in (pts[2] if c == L else pts.ravel())]))
        if rng.random() < 0.3:
            seq.append((Z, []))
        groups.append(seq)
    return groups


def crafted_split():
    return [
        ([[(M, [10, 20]), (L, [30, 40])]], "one_line"),
        ([[(M, [0, 0]), (L, [228, 0]), (L, [228, 228]), (L, [0, 228]), (Z, [])]], "long_lines_closed"),
        ([[(M, [10, 10]), (C, [10, 10, 10, 10, 10, 10]), (L, [50, 10])]], "cubic_of_length_zero"),
        ([[(M, [20, 200]), (C, [20, 20, 230, 20, 230, 200])], [(M, [5, 5]), (L, [7, 5]), (C, [8, 5, 9, 6, 9, 7])]],
         "long_and_short_cubic"),
        ([[(M, [1.5, 2.25]), (L, [100.75, 2.25]), (C, [120.5, 30.25, 90.125, 60.5, 100.75, 90.5]), (L, [1.5, 90.5]), (Z, [])],
          [], [(M, [200, 200]), (L, [200.5, 200.5])]], "float_coordinates_and_an_empty_group"),
    ]


def crafted_arcs():
    k = 0.0
    return [
        ([[(M, [50, 100]), (A, [50, 50, 0, 0, 1, 150, 100]), (A, [50, 50, 0, 0, 1, 50, 100]), (Z, [])]], "circle_two_semicircles"),
        ([[(M, [150, 100]), (A, [50, 50, 0, 0, 1, 100, 150])]], "quarter_arc"),
        ([[(M, [150, 100]), (A, [50, 50, 0, 1, 0, 100, 150])]], "three_quarter_arc"),
        ([[(M, [100, 60]), (A, [80, 40, 30, 0, 1, 160, 140]), (A, [80, 40, 30, 1, 0, 100, 60])]], "rotated_ellipse"),
        # (not right behind the `m`: the reference's `m` is written from the start point its first command object carries)
        ([[(M, [10, 10]), (L, [50, 20]), (A, [k, k, 0, 0, 1, 90, 40]), (L, [120, 40]), (A, [k, k, 45, 1, 1, 20, 200]),
           (L, [10, 10])]], "both_radii_zero_dropped"),
        ([[(M, [30, 30]), (L, [60, 90]), (A, [25, 40, 10, 1, 0, 60, 90]), (L, [90, 30]), (A, [10, 10, 0, 0, 0, 90, 30.0001])]],
         "start_equals_end_dropped"),
        ([[(M, [40, 40]), (A, [30, 60, 200, 0, 0, 80, 70]), (C, [90, 80, 100, 100, 120, 90]), (Z, [])],
          [(M, [200, 50]), (A, [30, 30, 0, 1, 1, 200, 110]), (L, [150, 80])]], "arc_cubic_close_and_a_semicircle_large_flag"),
    ]


def padded(results, n_icons):
    lo = max([len(c) for res in results for c, _ in res] + [1])
    oc = np.full((n_icons, G, lo), -2, np.int8)
    oa = np.full((n_icons, G, lo, 11), -1.0, np.float32)
    ln = np.zeros((n_icons, G), np.int32)
    for b, res in enumerate(results):
        for g, (c, a) in enumerate(res):
            ln[b, g] = len(c)
            oc[b, g, :len(c)] = c
            oa[b, g, :len(c)] = a
    return oc, oa, ln


def max_diff(expected, oc, oa, ln):
    """commands and counts must be equal; -> the largest absolute coordinate difference"""
    worst = 0.0
    for b in range(len(ln)):
        assert expected["valid"][b]
        for g in range(G):
            n = ln[b, g]
            assert expected["len_groups"][b, g] == n, (b, g, expected["len_groups"][b, g], n)
            assert np.array_equal(expected["commands"][b, g, 1:1 + n], oc[b, g, :n].astype(np.float32)), (b, g)
            e, r = expected["args"][b, g, 1:1 + n].astype(np.float64), oa[b, g, :n].astype(np.float64)
            # the slots the row's command enables (the reference also fills the start position, which is not among the eleven)
            live = ref.enabled(expected["commands"][b, g, 1:1 + n])
            if n:
                worst = max(worst, float(np.abs(e - r)[live].max(initial=0.0)))
    return worst


if __name__ == "__main__":
    rng = np.random.default_rng(2025)
    rec = {}

    # ---- split -----------------------------------------------------------------------------------------------------
    icons, rejected = list(crafted_split()), 0
    while len(icons) < 36:
        groups = random_split_icon(rng)
        if split_ok(*pack(groups)):
            icons.append((groups, "random"))
        else:
            rejected += 1
    for groups, tag in crafted_split():
        assert split_ok(*pack(groups)), tag
    cmds, args = zip(*[pack(groups) for groups, _ in icons])
    cmds, args = np.stack(cmds), np.stack(args)
    rec.update(split_commands=cmds, split_args=args, split_tags=np.array([t for _, t in icons]),
               split_lengths=np.stack([ref_lengths(c, a) for c, a in zip(cmds, args)]))
    worst = 0.0
    variants = [(f"n{n}", dict(n=n)) for n in NS]
    variants += [(f"{k}_{'lines' if il else 'nolines'}", dict(max_dist=d, include_lines=il)) for k, d in MAX_DISTS.items()
                 for il in (True, False)]
    for name, kw in variants:
        results = [run_reference(c, a, lambda p: p.split(**kw)) for c, a in zip(cmds, args)]
        oc, oa, ln = padded(results, len(icons))
        rec[f"split_{name}_commands"], rec[f"split_{name}_args"], rec[f"split_{name}_len"] = oc, oa, ln
        expected = ref.split(cmds.astype(np.float32), args, max_seq_len=oc.shape[2], **kw)
        worst = max(worst, max_diff(expected, oc, oa, ln))
        print("split", name, "LO", oc.shape[2], "rows", int(ln.sum()))
    rec["split_max_abs_diff"] = np.float64(worst)
    lens64 = np.stack([lengths64(c, a) for c, a in zip(cmds, args)])
    live = rec["split_lengths"] > 0
    assert np.array_equal(lens64 > 0, live)
    rel = np.abs(lens64 - rec["split_lengths"])[live] / np.maximum(rec["split_lengths"][live], 1.0)
    is_c = (cmds == C)[live]
    rec["length_max_rel_diff"] = np.float64(rel[is_c].max())          # `c`: float64 in the reference too
    rec["line_length_max_rel_diff"] = np.float64(rel[~is_c].max())    # `l`: the reference takes the float32 norm
    print("length diffs, relative to max(length, 1): c", rel[is_c].max(), "l", rel[~is_c].max())
    print("split:", len(icons), "icons,", rejected, "rejected near a boundary; max abs diff", worst, "length rel diff",
          float(rec["length_max_rel_diff"]))

    # ---- arcs ------------------------------------------------------------------------------------------------------
    icons, rejected = [], 0
    for groups, tag in crafted_arcs():
        assert arcs_ok(*pack(groups), exact=True), tag
        icons.append((groups, tag))
    while len(icons) < 36:
        groups = random_arc_icon(rng)
        if arcs_ok(*pack(groups), exact=False):
            icons.append((groups, "random"))
        else:
            rejected += 1
    cmds, args = zip(*[pack(groups) for groups, _ in icons])
    cmds, args = np.stack(cmds), np.stack(args)
    results = [run_reference(c, a, lambda p: p.simplify_arcs()) for c, a in zip(cmds, args)]
    oc, oa, ln = padded(results, len(icons))
    expected = ref.arcs_to_beziers(cmds.astype(np.float32), args, max_seq_len=oc.shape[2])
    worst = max_diff(expected, oc, oa, ln)
    for b in range(len(icons)):
        d = max_diff({k: v[b:b + 1] for k, v in expected.items()}, oc[b:b + 1], oa[b:b + 1], ln[b:b + 1])
        if d > 1e-3:
            print("  large difference:", b, icons[b][1], d)
    rec.update(arcs_commands=cmds, arcs_args=args, arcs_tags=np.array([t for _, t in icons]), arcs_out_commands=oc,
               arcs_out_args=oa, arcs_out_len=ln, arcs_max_abs_diff=np.float64(worst))
    n_arcs = int((cmds == A).sum())
    print("arcs:", len(icons), "icons,", n_arcs, "arcs,", rejected, "rejected; LO", oc.shape[2], "max abs diff", worst)
    for (groups, tag), res in zip(icons[:len(crafted_arcs())], results):
        print("  ", tag, [int((c == C).sum()) for c, _ in res])

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "expand.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")
