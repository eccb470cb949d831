"""Generates tests/golden/svgio/parse.npz by running the REAL reference parser, `deepsvg.svglib.svg_path.SVGPath.from_str(s)
.to_tensor()`, `SVGPolyline / SVGPolygon.from_xml(...).to_path().to_tensor()` and `SVG.from_str(document)` (imported read-only
from /root/reference), on path strings and small documents.  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_svgio.py

The reference's drawing stack is not installed here; those modules are stubbed with the stub list of make_golden_paths.py - the
parser itself only touches numpy, torch and `re`.  Stored:
 - the strings as bytes with offsets and kinds, and a tag per string naming what it covers;
 - for each string a flag: 0 rows, 1 the reference raises, 2 an empty group, 3 outside the kernel's fast number path (five named
   strings, and the `d` strings of the reference's docs/ that hold a 17-digit number above 2^53);
 - the reference's rows, reduced to the command and the model's eleven argument columns under CMD_ARGS_MASK;
 - six documents the generator writes itself, with the reference's per-group rows, `fill`, `filling` and view box.
No reference code and no reference file is stored: only path strings and result tensors."""
import glob
import os
import re
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
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

from deepsvg.svglib.svg import SVG                                         # noqa: E402
from deepsvg.svglib.svg_path import SVGPath                                # noqa: E402
from deepsvg.svglib.svg_primitive import SVGPolygon, SVGPolyline           # noqa: E402
from tests import svgio_ref as R                                           # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "svgio")
ARG_COLS = [1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13]      # the model's eleven argument columns of the 14-wide row
MASK = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1],
                 [1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1], [0] * 11, [0] * 11, [0] * 11], dtype=bool)
ROWS, RAISES, EMPTY, SLOW = range(4)
MAX_ROWS = 500                                        # strings of the docs with more rows are left out


def reduce(t):
    """the reference's [n, 14] tensor -> (commands int8 [n], args float32 [n, 11]) under CMD_ARGS_MASK"""
    t = t.numpy().astype(np.float32)
    cmd = t[:, 0].astype(np.int8)
    args = t[:, ARG_COLS].copy()
    args[~MASK[cmd]] = -1.0
    return cmd, args


class _Element:
    def __init__(self, points):
        self.points = points

    def hasAttribute(self, name):
        return False

    def getAttribute(self, name):
        return self.points


def reference(s, kind):
    """-> (flag, commands, args)"""
    none = (np.zeros(0, np.int8), np.zeros((0, 11), np.float32))
    try:
        if kind == R.KIND_PATH:
            group = SVGPath.from_str(s)
            if not group.svg_paths:
                return (EMPTY,) + none
        else:
            prim = (SVGPolygon if kind == R.KIND_POLYGON else SVGPolyline).from_xml(_Element(s))
            if len(prim.points) < 2:
                return (EMPTY,) + none                # no command: the reference has no tensor for it
            group = prim.to_path()
        return (ROWS,) + reduce(group.to_tensor())
    except (AssertionError, IndexError):
        return (RAISES,) + none


# ---- the strings ------------------------------------------------------------------------------------------------------------------
def doc_strings():
    """the `d` strings of the reference's docs/ -> (those whose numbers are all inside the fast path, the others).  Most of those
    files were written by the reference itself, float32 values printed through float64 with 16..17 digits; a string with a
    17-digit number above 2^53 is SLOW_NUMBER by definition and is stored with flag 3, so that the parity tests see that
    status on real data"""
    out, slow = [], []
    for f in sorted(glob.glob("/root/reference/docs/**/*.svg", recursive=True)):
        for d in re.findall(r'\sd="([^"]*)"', open(f, encoding="utf-8").read()):
            (out if fast(d, R.KIND_PATH) else slow).append(("docs" if fast(d, R.KIND_PATH) else "docs slow", d, R.KIND_PATH))
    return out, slow


class Grammar:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def number(self, style=None):
        r = self.rng
        style = r.randint(0, 10) if style is None else style
        v = r.randint(-300, 300)
        if style == 0:
            return str(v)
        if style == 1:
            return f"{v / 8:.3f}"
        if style == 2:
            return f"{abs(v) / 100:.2f}".lstrip("0") or ".0"       # .5
        if style == 3:
            return f"{abs(v)}."                                    # 5.
        if style == 4:
            return f"{v}e-{r.randint(0, 4)}"
        if style == 5:
            return "+" + str(abs(v))
        if style == 6:
            return "-0"
        if style == 7:
            return f"{r.uniform(-200, 200):.{r.randint(1, 7)}f}"
        if style == 8:
            return f"{v}E+{r.randint(0, 3)}"
        return f"{r.uniform(-1, 1) * 10.0 ** r.randint(-6, 6):.6g}"

    def sep(self):
        return [" ", ",", " , ", "\n", "\t", ""][self.rng.randint(0, 6)]

    def numbers(self, k):
        """k numbers with separators; a separator may be empty in front of a sign or a leading dot only"""
        out = ""
        for i in range(k):
            n = self.number()
            s = self.sep()
            if i and s == "" and n[0] not in "+-":
                s = " "
            out += s + n
        return out

    def path(self, n_letters, letters="MmZzLlHhVvCcSsQqTtAa", start="M"):
        out = start + self.numbers(2) if start else ""
        for _ in range(n_letters):
            c = letters[self.rng.randint(0, len(letters))]
            k = R.ARITY[c.lower()] * self.rng.randint(1, 4)
            out += self.sep() + c + self.numbers(k)
        return out


def grammar_strings():
    g = Grammar(20240611)
    P = R.KIND_PATH
    out = []
    for c in "MmLlHhVvCcSsQqTtAa":                                    # every letter in both cases, with an implicit repeat
        out.append((f"letter {c}", f"M10 20{c}" + g.numbers(2 * R.ARITY[c.lower()]) + "z", P))
    out += [("implicit line after move", "M1 2 3 4 5 6", P), ("implicit line after move", "m1 2 3 4 5 6z", P),
            ("s after bezier", "M0 0C1 2 3 4 5 6S7 8 9 10", P), ("s after line", "M0 0L5 6S7 8 9 10", P),
            ("t after bezier across letters", "M0 0C1 2 3 4 5 6T9 10", P), ("t after q", "M0 0q1 2 3 4t5 6t7 8", P),
            ("t after line", "M0 0l5 6t7 8", P), ("s after s", "M0 0s1 2 3 4 5 6 7 8", P), ("s after z", "M1 1c1 2 3 4 5 6zs1 2 3 4", P),
            ("t after arc", "M0 0a1 2 3 0 1 5 6t7 8", P), ("h and v", "M1 2h3v4H5V6h-1.5v.5", P),
            ("numbers", "M1.5.5 1-2L.5 5. 1e-3-0+7", P), ("numbers", "M10-2e1 4e 5L1. 2", P), ("numbers", "M4e+.5 1L1e5.5 1", P),
            ("numbers", "M--1-+2L+-3.4.5.6", P), ("numbers", "M1..5 2L3ee4 5e-", P), ("numbers", "M0.000 -0.0L00012.500 1e0", P),
            ("numbers", "M1e22 1e-22L123456789012345 0.000000000000001", P), ("negative zero", "M-0 -0.0l-0 0", P),
            ("junk", "M1 2 # L3;4 !?L5 6", P), ("junk", "xM1 2yL3 4", P), ("non-ascii", "M1 2éL3€4 ü", P),
            ("rows before the first move", "L1 2 3 4M5 6l1 1", P), ("rows before the first move", "c1 2 3 4 5 6h2M5 6t1 1", P),
            ("rows after z", "M1 1L2 2zL3 3l1 1M4 4l1 1", P), ("rows after z", "M1 1l2 2zc1 2 3 4 5 6zm1 1l1 1", P),
            ("M1 1z", "M1 1z", P), ("M M", "M M", P), ("empty", "", P), ("separators", " ,\n\t ,", P),
            ("numbers only", "1 2 3 4", P), ("numbers before the first letter", "1e999 7 M1 2L3 4", P),
            ("trailing letter", "M1 2L3 4L", P), ("count", "M1 2L3 4 5", P), ("count", "M1", P), ("count", "M1 2z5", P),
            ("count", "M1 2a1 1 0 01 2 2", P), ("count", "M1 2h", P), ("two closed", "M1 1l1 0 0 1zM5 5l1 0 0 1z", P),
            ("move move", "M1 1M2 2l1 1", P), ("arc flags", "M0 0A5 5 30 1.7 0.2 10 10a1 2 3 -1 2 4 5", P),
            ("zz", "M1 1l1 1zzl2 2", P), ("e is no letter", "M1 2e3 4", P), ("letters glued", "M1,2L3,4ZM5,6H7V8Z", P)]
    for i in range(6):                                                   # relative chains of 50 commands: float32 accumulation
        out.append(("relative chain", g.path(50, letters="lhvcsqta", start="m"), P))
    for i in range(40):
        out.append(("random", g.path(g.rng.randint(1, 12)), P))
    for i in range(10):
        out.append(("random from no move", g.path(g.rng.randint(1, 8), start=""), P))
    for kind in (R.KIND_POLYLINE, R.KIND_POLYGON):
        out += [("points", "1,2 3,4 5,6", kind), ("points odd", "1,2 3", kind), ("points one", "1 2", kind),
                ("points none", "", kind), ("points letters", "1 2L3 4z5 6e1 7", kind), ("points numbers", "1.5.5-2+3e1.5", kind)]
        for i in range(6):
            out.append(("points random", g.numbers(2 * g.rng.randint(2, 20)), kind))
    return out


SLOW_STRINGS = [("slow: 17 digits", "M0.12345678901234567 1L2 3"), ("slow: 2^53", "M9007199254740992 1L2 3"),
                ("slow: exponent", "M1e23 1L2 3"), ("slow: small", "M1 2L1e-30 3"), ("slow: 25 digits", "M1 2l1234567890123456789012345 1")]


def fast(s, kind):
    """every number the reference converts is inside the fast path"""
    data = s.encode("utf-8")
    seen = kind != R.KIND_PATH
    for tok in R.tokens(data, kind):
        if tok[0] == "c":
            seen = True
        elif seen and R.decimal(data[tok[1]:tok[2]]) is None:
            return False
    return True


# ---- the documents ------------------------------------------------------------------------------------------------------------------
DOCS = [
    '<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 24 24"><path d="M1 2L3 4C5 6 7 8 9 10z" fill="none" filling="1"/>'
    '<path d="M12 12l1 1 1-1z" filling="2"/></svg>',
    '<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 100 100"><rect x="10" y="20.5" width="30" height="40"/>'
    '<circle cx="50" cy="50" r="12.5" fill="none"/><ellipse cx="20" cy="30" rx="5" ry="7.25"/>'
    '<line x1="1" y1="2" x2="3.5" y2="4"/><polyline points="1,2 3,4 5,6.5" fill="none"/><polygon points="10 10 20 10 15 20"/></svg>',
    '<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 48 48"><g><g><path d="M1 1h5v5z"/></g><rect width="4" height="5"/></g>'
    '<path d="m2 2 3 3"/><g fill="none"><circle cx="1.5" cy="-2.5" r="0.1"/></g></svg>',
    '<svg xmlns="http://www.w3.org/2000/svg" viewBox="-12.5 8 64 64"><path d="M-10 10L50 70a5 6 7 1 0 3 3" filling="1"/>'
    '<line x2="5" y2="6"/></svg>',
    '<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 200 100"><path d="M0 0L200 100"/><path d="M5 5"/>'
    '<polygon points="0,0 200,0 200,100" fill="none"/></svg>',
    '<svg xmlns="http://www.w3.org/2000/svg" viewBox="3 4 30 60.5"><ellipse cx="10" cy="20" rx="0.1" ry="0.7" fill="none"/>'
    '<rect x="-1" y="-2" width="0.3" height="0.1" fill="red"/><path d="M1 1q1 1 2 2t1 1" fill="none" filling="2"/></svg>',
]


def document(text):
    svg = SVG.from_str(text)
    groups = [g.to_path() for g in svg.svg_path_groups]
    rows = [reduce(g.to_tensor()) if g.svg_paths else (np.zeros(0, np.int8), np.zeros((0, 11), np.float32)) for g in groups]
    fill = [bool(g.fill) for g in svg.svg_path_groups]
    filling = [int(g.svg_paths[0].filling) if g.svg_paths else 0 for g in groups]
    vb = np.array([*svg.viewbox.xy.pos, *svg.viewbox.wh.pos], dtype=np.float32)
    return rows, fill, filling, vb


def main():
    os.makedirs(OUT, exist_ok=True)
    docs_fast, docs_slow = doc_strings()
    entries, long_rows = [], 0
    for tag, s, kind in docs_fast + grammar_strings():
        flag, cmd, args = reference(s, kind)
        if len(cmd) > MAX_ROWS:
            long_rows += 1
            continue
        assert fast(s, kind), (tag, s)
        entries.append((tag, s, kind, flag, cmd, args))
    none = (np.zeros(0, np.int8), np.zeros((0, 11), np.float32))
    for tag, s in SLOW_STRINGS:                          # the five named strings: the only made-up ones outside the fast path
        assert not fast(s, R.KIND_PATH), s
        assert reference(s, R.KIND_PATH)[0] == ROWS
        entries.append((tag, s, R.KIND_PATH, SLOW) + none)
    for tag, s, kind in docs_slow:
        assert reference(s, kind)[0] == ROWS             # the reference reads them; the kernel's fast path does not
        entries.append((tag, s, kind, SLOW) + none)
    print(f"docs: {len(docs_fast)} strings inside the fast path, {len(docs_slow)} outside it (stored with flag 3); {long_rows} "
          f"strings with more than {MAX_ROWS} rows left out")
    raw = [e[1].encode("utf-8") for e in entries]
    out = {
        "data": np.frombuffer(b"".join(raw), dtype=np.uint8),
        "offsets": np.cumsum([0] + [len(r) for r in raw]).astype(np.int64),
        "kind": np.array([e[2] for e in entries], dtype=np.uint8),
        "flag": np.array([e[3] for e in entries], dtype=np.uint8),
        "tag": np.array([e[0] for e in entries]),
        "row_offsets": np.cumsum([0] + [len(e[4]) for e in entries]).astype(np.int64),
        "commands": np.concatenate([e[4] for e in entries]),
        "args": np.concatenate([e[5] for e in entries]),
        "left_out_long": np.int64(long_rows),             # strings left out for having more than MAX_ROWS rows
    }
    docs = [document(t) for t in DOCS]
    draw = [d.encode("utf-8") for d in DOCS]
    out["doc_data"] = np.frombuffer(b"".join(draw), dtype=np.uint8)
    out["doc_offsets"] = np.cumsum([0] + [len(d) for d in draw]).astype(np.int64)
    out["doc_group_offsets"] = np.cumsum([0] + [len(d[0]) for d in docs]).astype(np.int64)
    groups = [g for d in docs for g in d[0]]
    out["doc_row_offsets"] = np.cumsum([0] + [len(g[0]) for g in groups]).astype(np.int64)
    out["doc_commands"] = np.concatenate([g[0] for g in groups])
    out["doc_args"] = np.concatenate([g[1] for g in groups])
    out["doc_fill"] = np.array([f for d in docs for f in d[1]], dtype=bool)
    out["doc_filling"] = np.array([f for d in docs for f in d[2]], dtype=np.int32)
    out["doc_viewbox"] = np.stack([d[3] for d in docs])
    np.savez_compressed(os.path.join(OUT, "parse.npz"), **out)
    flags = out["flag"]
    print(f"{len(entries)} strings ({sum(len(r) for r in raw)} bytes, {len(out['commands'])} rows): "
          f"{(flags == ROWS).sum()} with rows, {(flags == RAISES).sum()} raise, {(flags == EMPTY).sum()} empty, "
          f"{(flags == SLOW).sum()} slow; {len(DOCS)} documents with {len(groups)} groups; "
          f"{os.path.getsize(os.path.join(OUT, 'parse.npz'))} bytes")


if __name__ == "__main__":
    main()
